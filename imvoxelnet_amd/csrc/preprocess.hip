// Device-side image pipeline (include/imvoxel.h, ivx_image_prep_u8): uint8 HWC BGR frames -> Resize -> Normalize -> Pad as ONE
// memory-bound launch that writes the fp32 NCHW tensor data.prepare_image builds on the host, bit for bit.
//
// Reference: configs/imvoxelnet/imvoxelnet_kitti.py:94-105 (Resize keep_ratio -> Normalize -> Pad(size_divisor=32)); the resize is the
// integer restatement of cv2.resize(INTER_LINEAR) on uint8 that data.imresize_cv2_linear / data._linear_tables hold (11-bit weights,
// int32 horizontal pass, `>> 4 ... >> 16 ... + 2 >> 2` vertical pass, the exact-half INTER_AREA shortcut).  Parity with cv2 itself is
// UNPINNED (cv2 is not available where this was written): the kernel is held to the host restatement, not to OpenCV.
//
// Layout: one thread produces 4 consecutive output x of one output row for all three planes (three 16-byte stores; scalar stores when
// pad_w % 4 != 0 or `out` is not 16-byte aligned).  It recomputes the horizontal pass on its two source rows, so there is no
// intermediate image; the pad region (y >= dst_h or x >= dst_w) is written as +0.0f by the same thread.  Work items are numbered x
// fastest, then y, then frame, so neighbouring workgroups read the same or adjacent source rows; capped grid, grid-stride loop.
// The per-axis coefficients are recomputed per item (one fp64 multiply / subtract per position and a few fp32 ops): no tables, no
// second launch, nothing for a C caller to prepare.
//
// Exactness (this file is built with -ffp-contract=off): fx is formed in fp64 as (d + 0.5) * (src / dst) - 0.5 with a separately
// rounded product (an fma changes results) and rounded once to fp32; everything after it is fp32 ops that are exact or rounded as
// numpy rounds them, then integers.  The normalisation is one fp32 subtract and one correctly rounded fp32 divide (hipcc's default).
#include "ivx_common.h"

#include <math.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { PREP_COPY = 0, PREP_AREA2 = 1, PREP_LINEAR = 2 };
constexpr int kPrepMaxDim = 32768;       // every extent (include/imvoxel.h IVX_IMAGE_PREP_MAX_DIM)
constexpr int kPrepMaxFrames = 1 << 20;
constexpr int kPrepGridCap = 2048;       // 256 CUs x 8 workgroups; larger batches stride

struct PrepP {
  const uint8_t *src;
  float *out;
  long long src_image_bytes, total;      // total = n * pad_h * qw work items
  double scale_x, scale_y;               // double(src) / double(dst)
  int src_h, src_w, row_bytes, dst_h, dst_w, pad_h, pad_w, qw, mode;
  int swap;                              // to_rgb: output channel c reads source channel 2 - c
  float mean[3], std[3];
};

// data._linear_tables for one output position: first source index, second source index, weights (a0 on s0, a1 on s1)
__device__ __forceinline__ void linear_coef(const int d, const double scale, const int src, int &s0, int &s1, int &a0, int &a1) {
  const float fx = (float)__dsub_rn(__dmul_rn((double)d + 0.5, scale), 0.5);
  const float fl = floorf(fx);
  int s = (int)fl;
  float f = __fsub_rn(fx, fl);
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= src - 1) { s = src - 1; f = 0.f; }
  s0 = s;
  s1 = min(s + 1, src - 1);
  a1 = (int)rintf(__fmul_rn(f, 2048.0f));                       // cvRound: half to even
  a0 = (int)rintf(__fmul_rn(__fsub_rn(1.0f, f), 2048.0f));
}

template <bool VEC>
__global__ __launch_bounds__(256) void image_prep_u8_kernel(const PrepP p) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int per_img = p.pad_h * p.qw;
  const long long plane = (long long)p.pad_h * p.pad_w;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += stride) {
    const int img = (int)(idx / per_img);
    const int rem = (int)(idx - (long long)img * per_img);
    const int y = rem / p.qw, x0 = (rem - y * p.qw) * 4;
    int v[3][4];                          // resized uint8 values [output channel][x]
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) v[c][j] = 0;
    if (y < p.dst_h && x0 < p.dst_w) {
      const uint8_t *s = p.src + (long long)img * p.src_image_bytes;
      if (p.mode == PREP_COPY) {
        const uint8_t *r = s + (long long)y * p.row_bytes;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int x = min(x0 + j, p.dst_w - 1);               // x >= dst_w is discarded below
#pragma unroll
          for (int c = 0; c < 3; ++c) v[c][j] = r[x * 3 + (p.swap ? 2 - c : c)];
        }
      } else if (p.mode == PREP_AREA2) {
        const uint8_t *r0 = s + (long long)(2 * y) * p.row_bytes, *r1 = r0 + p.row_bytes;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int o = 6 * min(x0 + j, p.dst_w - 1);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int k = o + (p.swap ? 2 - c : c);
            v[c][j] = (r0[k] + r0[k + 3] + r1[k] + r1[k + 3] + 2) >> 2;
          }
        }
      } else {
        int sy0, sy1, b0, b1;
        linear_coef(y, p.scale_y, p.src_h, sy0, sy1, b0, b1);
        const uint8_t *r0 = s + (long long)sy0 * p.row_bytes, *r1 = s + (long long)sy1 * p.row_bytes;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          int sx0, sx1, a0, a1;
          linear_coef(min(x0 + j, p.dst_w - 1), p.scale_x, p.src_w, sx0, sx1, a0, a1);
          sx0 *= 3;
          sx1 *= 3;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int k = p.swap ? 2 - c : c;
            const int d0 = r0[sx0 + k] * a0 + r0[sx1 + k] * a1;          // <= 255 * 2048
            const int d1 = r1[sx0 + k] * a0 + r1[sx1 + k] * a1;
            const int q = (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2;
            v[c][j] = min(max(q, 0), 255);
          }
        }
      }
    }
    float *o = p.out + (long long)img * 3 * plane + (long long)y * p.pad_w + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float m = p.mean[c], sd = p.std[c];
      f32x4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[j] = (y < p.dst_h && x0 + j < p.dst_w) ? __fsub_rn((float)v[c][j], m) / sd : 0.f;
      }
      if (VEC) {
        *reinterpret_cast<f32x4 *>(o + c * plane) = r;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < p.pad_w) o[c * plane + j] = r[j];
      }
    }
  }
}

}  // namespace

// mmcv.rescale_size for a (long, short) scale, as data.rescale_size: f = min(max_long / max(h, w), max_short / min(h, w)) in double,
// size = int(h * f + 0.5).  Host only.
extern "C" int ivx_rescale_size(int32_t src_h, int32_t src_w, int32_t scale_a, int32_t scale_b, int32_t *dst_h, int32_t *dst_w) {
  IVX_REQUIRE(dst_h && dst_w, "ivx_rescale_size: null argument");
  IVX_REQUIRE(src_h > 0 && src_w > 0 && scale_a > 0 && scale_b > 0, "ivx_rescale_size: sizes must be positive (got %d x %d, scale (%d, %d))", src_h,
              src_w, scale_a, scale_b);
  const double max_long = scale_a > scale_b ? scale_a : scale_b, max_short = scale_a > scale_b ? scale_b : scale_a;
  const double lng = src_h > src_w ? src_h : src_w, sht = src_h > src_w ? src_w : src_h;
  const double f0 = max_long / lng, f1 = max_short / sht;
  const double f = f0 < f1 ? f0 : f1;
  const double h = (double)src_h * f + 0.5, w = (double)src_w * f + 0.5;
  IVX_REQUIRE(h < 2147483647.0 && w < 2147483647.0, "ivx_rescale_size: %d x %d at scale (%d, %d) overflows int32", src_h, src_w, scale_a, scale_b);
  *dst_h = (int32_t)h;
  *dst_w = (int32_t)w;
  return IVX_OK;
}

extern "C" int ivx_image_prep_u8(const ivx_image_prep_desc *d, const void *src, int64_t src_image_bytes, int32_t n, float *out,
                                 ivx_stream_t stream) {
  IVX_REQUIRE(d && src && out, "ivx_image_prep_u8: null argument");
  IVX_REQUIRE(d->src_h > 0 && d->src_w > 0 && d->dst_h > 0 && d->dst_w > 0, "ivx_image_prep_u8: sizes must be positive (src %d x %d, dst %d x %d)",
              d->src_h, d->src_w, d->dst_h, d->dst_w);
  IVX_REQUIRE(d->pad_h >= d->dst_h && d->pad_w >= d->dst_w, "ivx_image_prep_u8: pad %d x %d is smaller than dst %d x %d", d->pad_h, d->pad_w,
              d->dst_h, d->dst_w);
  IVX_REQUIRE(d->src_h <= kPrepMaxDim && d->src_w <= kPrepMaxDim && d->pad_h <= kPrepMaxDim && d->pad_w <= kPrepMaxDim,
              "ivx_image_prep_u8: extents above %d are not supported (src %d x %d, pad %d x %d)", kPrepMaxDim, d->src_h, d->src_w, d->pad_h, d->pad_w);
  IVX_REQUIRE((int64_t)d->src_row_bytes >= 3 * (int64_t)d->src_w, "ivx_image_prep_u8: src_row_bytes %d is below 3 * src_w = %d", d->src_row_bytes,
              3 * d->src_w);
  for (int c = 0; c < 3; ++c)
    IVX_REQUIRE(isfinite(d->std[c]) && d->std[c] != 0.f, "ivx_image_prep_u8: std[%d] = %g must be finite and non-zero", c, (double)d->std[c]);
  IVX_REQUIRE(n > 0 && n <= kPrepMaxFrames, "ivx_image_prep_u8: n = %d must be in 1 .. %d", n, kPrepMaxFrames);
  IVX_REQUIRE(n == 1 || src_image_bytes >= (int64_t)d->src_h * d->src_row_bytes,
              "ivx_image_prep_u8: src_image_bytes %lld is below src_h * src_row_bytes = %lld", (long long)src_image_bytes,
              (long long)d->src_h * d->src_row_bytes);
  PrepP p;
  p.src = (const uint8_t *)src;
  p.out = out;
  p.src_image_bytes = n == 1 ? 0 : src_image_bytes;
  p.src_h = d->src_h, p.src_w = d->src_w, p.row_bytes = d->src_row_bytes;
  p.dst_h = d->dst_h, p.dst_w = d->dst_w, p.pad_h = d->pad_h, p.pad_w = d->pad_w;
  p.qw = (d->pad_w + 3) / 4;
  p.total = (long long)n * d->pad_h * p.qw;
  p.scale_x = (double)d->src_w / (double)d->dst_w;
  p.scale_y = (double)d->src_h / (double)d->dst_h;
  // the order of data.imresize_cv2_linear: equal size is a copy, an exact half on BOTH axes the INTER_AREA mean, the tables otherwise
  p.swap = d->to_rgb != 0;
  p.mode = (d->src_h == d->dst_h && d->src_w == d->dst_w)           ? PREP_COPY
           : (d->src_h == 2 * d->dst_h && d->src_w == 2 * d->dst_w) ? PREP_AREA2
                                                                    : PREP_LINEAR;
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = d->mean[c];
    p.std[c] = d->std[c];
  }
  long long blocks = (p.total + 255) / 256;
  if (blocks > kPrepGridCap) blocks = kPrepGridCap;
  const bool vec = d->pad_w % 4 == 0 && ((uintptr_t)out & 15) == 0;
  if (vec) hipLaunchKernelGGL(image_prep_u8_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(image_prep_u8_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  IVX_CHECK_LAUNCH("ivx_image_prep_u8");
  return IVX_OK;
}
