// Device-side image pipeline (include/imvoxel.h, ivx_image_prep_u8): uint8 HWC BGR frames -> Resize -> Normalize -> Pad as ONE
// memory-bound launch that writes the fp32 NCHW tensor data.prepare_image builds on the host, bit for bit.
//
// Since 0.5.3 also ivx_image_prep_fmt_u8: the same launch on frames in a decoder's pixel format (RGB, BGRA / RGBA, gray, NV12, YUYV), converted
// to BGR inside the fetch (pixel_fetch.h), and ivx_yuv_matrix, the named integer matrices.
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
#include "pixel_fetch.h"

#include <math.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { PREP_COPY = 0, PREP_AREA2 = 1, PREP_LINEAR = 2 };
struct PrepP {
  const uint8_t *src;
  float *out;
  long long src_image_bytes, total;      // total = n * pad_h * qw work items
  double scale_x, scale_y;               // double(src) / double(dst)
  int dst_h, dst_w, pad_h, pad_w, qw, mode;  // (the source geometry is PixSrc's)
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

// The one kernel of this file, for every pixel layout (0.5.3): the source access is a fetch policy (pixel_fetch.h) that returns a pixel's
// three BGR bytes.  A tap is fetched (and, for the YUV layouts, converted) ONCE and the three output channels pick from it; the copy and the
// exact-half paths read their consecutive columns as even-aligned pairs, which share a chroma pair in NV12 and YUYV.  ivx_image_prep_u8
// launches the BGR8 instantiation (same bits as the kernel it had before, tests/golden/image_prep_bgr_0_5_2.npz; 0.76 .. 0.82 of its time,
// profiles/image_prep_fmt.md).
template <int L, bool VEC>
__global__ __launch_bounds__(256) void image_prep_fmt_u8_kernel(const PrepP p, const PixSrc f) {
  typedef PixFetch<L> F;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int per_img = p.pad_h * p.qw;
  const long long plane = (long long)p.pad_h * p.pad_w;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += stride) {
    const int img = (int)(idx / per_img);
    const int rem = (int)(idx - (long long)img * per_img);
    const int y = rem / p.qw, x0 = (rem - y * p.qw) * 4;
    int v[4][3];                          // resized uint8 values [x][BGR]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) v[j][k] = 0;
    if (y < p.dst_h && x0 < p.dst_w) {
      const uint8_t *s = p.src + (long long)img * p.src_image_bytes;
      if (p.mode == PREP_COPY) {                                  // columns past dst_w - 1 are clamped by pair() and discarded below
        F::pair(f, s, x0, y, v[0], v[1]);
        F::pair(f, s, x0 + 2, y, v[2], v[3]);
      } else if (p.mode == PREP_AREA2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int x = 2 * min(x0 + j, p.dst_w - 1);               // src_w == 2 * dst_w: both columns exist
          int a[3], b[3], c[3], d[3];
          F::pair(f, s, x, 2 * y, a, b);
          F::pair(f, s, x, 2 * y + 1, c, d);
#pragma unroll
          for (int k = 0; k < 3; ++k) v[j][k] = (a[k] + b[k] + c[k] + d[k] + 2) >> 2;
        }
      } else {
        int sy0, sy1, b0, b1;
        linear_coef(y, p.scale_y, f.src_h, sy0, sy1, b0, b1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          int sx0, sx1, a0, a1;
          linear_coef(min(x0 + j, p.dst_w - 1), p.scale_x, f.src_w, sx0, sx1, a0, a1);
          int t00[3], t01[3], t10[3], t11[3];
          F::px(f, s, sx0, sy0, t00);
          F::px(f, s, sx1, sy0, t01);
          F::px(f, s, sx0, sy1, t10);
          F::px(f, s, sx1, sy1, t11);
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const int d0 = t00[k] * a0 + t01[k] * a1;                    // <= 255 * 2048
            const int d1 = t10[k] * a0 + t11[k] * a1;
            const int q = (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2;
            v[j][k] = min(max(q, 0), 255);
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
        const int b = p.swap ? v[j][2 - c] : v[j][c];
        r[j] = (y < p.dst_h && x0 + j < p.dst_w) ? __fsub_rn((float)b, m) / sd : 0.f;
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

// Fill the kernel's parameters from a checked call and launch the layout's instantiation (declared in pixel_fetch.h; what: the entry's name).
int ivx_image_prep_launch(const ivx_image_prep_desc *d, int32_t layout, const PixSrc &f, const void *src, int64_t src_image_bytes, int32_t n, float *out,
                          ivx_stream_t stream, const char *what) {
  PrepP p;
  p.src = (const uint8_t *)src;
  p.out = out;
  p.src_image_bytes = n == 1 ? 0 : src_image_bytes;
  p.dst_h = d->dst_h, p.dst_w = d->dst_w, p.pad_h = d->pad_h, p.pad_w = d->pad_w;
  p.qw = (d->pad_w + 3) / 4;
  p.total = (long long)n * d->pad_h * p.qw;
  p.scale_x = (double)d->src_w / (double)d->dst_w;
  p.scale_y = (double)d->src_h / (double)d->dst_h;
  p.swap = d->to_rgb != 0;
  // the order of data.imresize_cv2_linear: equal size is a copy, an exact half on BOTH axes the INTER_AREA mean, the tables otherwise
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
#define IVX_PREP_LAUNCH(L)                                                                                                         \
  if (vec) hipLaunchKernelGGL((image_prep_fmt_u8_kernel<L, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, f); \
  else hipLaunchKernelGGL((image_prep_fmt_u8_kernel<L, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, f)
  IVX_PIX_DISPATCH(layout, IVX_PREP_LAUNCH)
#undef IVX_PREP_LAUNCH
  IVX_CHECK_LAUNCH(what);
  return IVX_OK;
}

extern "C" int ivx_image_prep_fmt_u8(const ivx_image_prep_desc *d, const ivx_frame_format *fmt, const ivx_lens *lens, const void *src,
                                     int64_t src_image_bytes, int32_t n, float *out, ivx_stream_t stream) {
  static const char *const what = "ivx_image_prep_fmt_u8";
  IVX_REQUIRE(d && src && out, "ivx_image_prep_fmt_u8: null argument");
  IVX_REQUIRE(fmt, "ivx_image_prep_fmt_u8: null frame format");
  IVX_REQUIRE(fmt->layout >= 0 && fmt->layout < IVX_PIX_COUNT, "ivx_image_prep_fmt_u8: unknown layout %d (IVX_PIX_BGR8 = 0 .. IVX_PIX_YUYV = 6)", fmt->layout);
  if (int e = prep_check_sizes(d, n, what)) return e;
  if (int e = prep_check_rows(d, fmt->layout, what)) return e;
  PixSrc f;
  if (int e = pix_src_fill(f, d, fmt, src, src_image_bytes, n, what)) return e;
  if (lens) return ivx_image_prep_lens_launch(d, fmt->layout, f, lens, src, src_image_bytes, n, out, stream, what);
  return ivx_image_prep_launch(d, fmt->layout, f, src, src_image_bytes, n, out, stream, what);
}

namespace {
// num / den (den > 0) rounded half to even, in integers
int64_t div_half_even(const int64_t num, const int64_t den) {
  int64_t q = num / den, r = num % den;
  if (r < 0) { q -= 1; r += den; }                  // floor
  if (2 * r > den || (2 * r == den && (q & 1))) q += 1;
  return q;
}
}  // namespace

// The integer YUV -> BGR matrix of a named standard (include/imvoxel.h).  Host only.  BT.601 limited range is OpenCV's table by value; the
// other rows are the exact rational matrix times 2^20, rounded half to even (Kr, Kb in ten-thousandths, so everything is an int64 ratio).
extern "C" int ivx_yuv_matrix(int32_t standard, int32_t full_range, ivx_frame_format *f) {
  IVX_REQUIRE(f, "ivx_yuv_matrix: null argument");
  IVX_REQUIRE(standard == IVX_YUV_BT601 || standard == IVX_YUV_BT709, "ivx_yuv_matrix: unknown standard %d (IVX_YUV_BT601 = 0, IVX_YUV_BT709 = 1)", standard);
  if (standard == IVX_YUV_BT601 && !full_range) {
    f->y_off = 16, f->cy = 1220542, f->cub = 2116026, f->cug = -409993, f->cvg = -852492, f->cvr = 1673527;
    return IVX_OK;
  }
  const int64_t D = 10000, kr = standard == IVX_YUV_BT601 ? 2990 : 2126, kb = standard == IVX_YUV_BT601 ? 1140 : 722, kg = D - kr - kb;
  const int64_t sn = full_range ? 1 : 255, sd = full_range ? 1 : 224, one = (int64_t)1 << 20;
  f->y_off = full_range ? 0 : 16;
  f->cy = (int32_t)(full_range ? one : div_half_even(255 * one, 219));
  f->cvr = (int32_t)div_half_even(2 * sn * (D - kr) * one, sd * D);
  f->cub = (int32_t)div_half_even(2 * sn * (D - kb) * one, sd * D);
  f->cug = (int32_t)div_half_even(-2 * sn * kb * (D - kb) * one, sd * D * kg);
  f->cvg = (int32_t)div_half_even(-2 * sn * kr * (D - kr) * one, sd * D * kg);
  return IVX_OK;
}

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
  static const char *const what = "ivx_image_prep_u8";
  IVX_REQUIRE(d && src && out, "ivx_image_prep_u8: null argument");
  if (int e = prep_check_sizes(d, n, what)) return e;
  if (int e = prep_check_rows(d, IVX_PIX_BGR8, what)) return e;
  IVX_REQUIRE(n == 1 || src_image_bytes >= (int64_t)d->src_h * d->src_row_bytes,
              "ivx_image_prep_u8: src_image_bytes %lld is below src_h * src_row_bytes = %lld", (long long)src_image_bytes,
              (long long)d->src_h * d->src_row_bytes);
  return ivx_image_prep_launch(d, IVX_PIX_BGR8, pix_src_bgr8(d), src, src_image_bytes, n, out, stream, what);
}
