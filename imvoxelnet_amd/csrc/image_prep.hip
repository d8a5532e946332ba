// Device-side image pipeline (include/imvoxel.h): uint8 frames -> [Undistort ->] Resize -> Normalize -> Pad as ONE memory-bound launch that
// writes the fp32 NCHW network input, and the cover / depth maps of the same geometry at feature resolution.
//   ivx_image_prep_u8        packed BGR frames, bit for bit the tensor data.prepare_image builds on the host
//   ivx_image_prep_lens_u8   the same frames of a real camera, undistorted in the launch (0.5.2)
//   ivx_image_prep_fmt_u8    either of the two on frames in a decoder's pixel format (RGB, BGRA / RGBA, gray, NV12, YUYV), converted to BGR
//                            inside the fetch (pixel_fetch.h), and ivx_yuv_matrix, the named integer matrices (0.5.3)
//   ivx_map_prep_lens        the maps (0.5.2);  ivx_rescale_size: mmcv's rescale rule on the host
// The file is one kernel skeleton with two samplers in it, one launcher and one checked path behind the three image entries; how the bytes of
// a frame lie is pixel_fetch.h's business alone.
//
// Skeleton (image_prep_kernel): one thread produces 4 consecutive output x of one output row for all three planes (three 16-byte stores;
// scalar stores when pad_w % 4 != 0 or `out` is not 16-byte aligned); the pad region (y >= dst_h or x >= dst_w) and the lens's border are
// written as +0.0f by the same thread.  Work items are numbered x fastest, then y, then frame, so neighbouring workgroups read the same or
// adjacent source rows; capped grid, grid-stride loop.  A sampler fills the thread's 4 x 3 BGR values and says which of the 4 pixels show
// the frame; the skeleton swaps channels, normalises (one fp32 subtract and one correctly rounded fp32 divide, hipcc's default) and stores.
// Every source access is a fetch policy PixFetch<L> that returns a pixel's three BGR bytes: a tap is fetched (and, for the YUV layouts,
// converted) ONCE and the three output channels pick from it.  The BGR entries launch the BGR8 instantiations (same bits as the kernels they
// had before 0.5.3, tests/golden/image_prep_bgr_0_5_2.npz; 0.76 .. 0.82 of their time plain, 0.79 .. 0.89 through a lens,
// profiles/image_prep_fmt.md).
//
// Resize sampler.  Reference: configs/imvoxelnet/imvoxelnet_kitti.py:94-105 (Resize keep_ratio -> Normalize -> Pad(size_divisor=32)); the
// resize is the integer restatement of cv2.resize(INTER_LINEAR) on uint8 that data.imresize_cv2_linear / data._linear_tables hold (11-bit
// weights, int32 horizontal pass, `>> 4 ... >> 16 ... + 2 >> 2` vertical pass, the exact-half INTER_AREA shortcut).  Parity with cv2 itself
// is UNPINNED (cv2 is not available where this was written): the kernel is held to the host restatement, not to OpenCV.  A thread
// recomputes the horizontal pass on its two source rows, so there is no intermediate image; the per-axis coefficients are recomputed per item
// (one fp64 multiply / subtract per position and a few fp32 ops): no tables, no second launch, nothing for a C caller to prepare.  The copy
// and the exact-half paths read their consecutive columns as even-aligned pairs, which share a chroma pair in NV12 and YUYV.
// Exactness (this file is built with -ffp-contract=off): fx is formed in fp64 as (d + 0.5) * (src / dst) - 0.5 with a separately rounded
// product (an fma changes results) and rounded once to fp32; everything after it is fp32 ops that are exact or rounded as numpy rounds them,
// then integers 0 .. 255, whose conversion to fp32 is exact.
//
// Lens sampler.  One geometric map G (the header writes every step) takes a pixel of the network input back to the raw frame: the resize's
// pixel-centre rule, the ideal camera new_K backwards, the distortion polynomial (OpenCV's 5-coefficient Brown model or its equidistant
// fisheye model) forwards, the real camera K.  G is evaluated once per pixel in fp64, each operation rounded on its own (-ffp-contract=off
// again, and the host reference restates the same order), so the coordinates of the kernel and of an fp64 reference agree to a few ulp of
// fp64 and every decision (inside / border, which four taps, which nearest pixel) can be made robust by the reference alone.  The blend
// after it is fp32 in the header's order; the fractions are rounded once.  The gather reads 2 x 2 taps per pixel; neighbouring lanes map to
// neighbouring source pixels (G is smooth), so a wavefront's taps fall into a few source rows and the cache lines are shared as in the
// resize.
// Map kernel: one lane per feature pixel; tiny and launch-bound.  No LDS, no atomics, plain vector stores.
#include "ivx_common.h"
#include "pixel_fetch.h"

#include <math.h>
#include <type_traits>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPrepMaxDim = 32768;       // every extent (include/imvoxel.h IVX_IMAGE_PREP_MAX_DIM)
constexpr int kPrepMaxFrames = 1 << 20;
constexpr int kPrepGridCap = 2048;       // 256 CUs x 8 workgroups; larger batches stride

struct PrepP {                           // what the skeleton needs (the source geometry is PixSrc's)
  const uint8_t *src;
  float *out;
  long long src_image_bytes, total;      // total = n * pad_h * qw work items
  int dst_h, dst_w, pad_h, pad_w, qw;
  int swap;                              // to_rgb: output channel c reads source channel 2 - c
  float mean[3], std[3];
};

enum { PREP_COPY = 0, PREP_AREA2 = 1, PREP_LINEAR = 2 };
struct ResizeP {
  double scale_x, scale_y;               // double(src) / double(dst)
  int mode;
};

struct LensG {                           // what G needs: the lens (model < 0: the ideal camera) and the resize
  int model;
  int src_h, src_w;
  double scale_x, scale_y;               // double(src) / double(dst)
  double fx, fy, cx, cy, k[5], nfx, nfy, ncx, ncy, r2_max;
  double u_hi, v_hi;                     // src_w - 0.5, src_h - 0.5
};

struct LensMapP {
  LensG g;
  const uint8_t *src;                    // nullptr: the cover map
  float *out;
  long long row_bytes, map_bytes, total; // total = n * fh * fw
  int dst_h, dst_w, fh, fw, stride, u16;
  float scale;
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

// the resize's own pixel-centre rule for one axis
__device__ __forceinline__ double centre(const int d, const double scale) { return __dsub_rn(__dmul_rn((double)d + 0.5, scale), 0.5); }

// G of the header for the source position (px, py) of one input pixel: (u, v) and the inside decision, in the header's operation order
__device__ __forceinline__ bool lens_map(const LensG &g, const double px, const double py, double &u, double &v) {
  if (g.model < 0) {
    u = px;
    v = py;
    return u >= -0.5 && u <= g.u_hi && v >= -0.5 && v <= g.v_hi;
  }
  const double xn = (px - g.ncx) / g.nfx, yn = (py - g.ncy) / g.nfy;
  const double r2 = xn * xn + yn * yn;
  double xd, yd;
  if (g.model == IVX_LENS_BROWN) {
    const double k1 = g.k[0], k2 = g.k[1], p1 = g.k[2], p2 = g.k[3], k3 = g.k[4];
    const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
    xd = (xn * rad + ((2.0 * p1) * xn) * yn) + p2 * (r2 + (2.0 * xn) * xn);
    yd = (yn * rad + p1 * (r2 + (2.0 * yn) * yn)) + ((2.0 * p2) * xn) * yn;
  } else {
    const double r = __dsqrt_rn(r2), th = atan(r), t2 = th * th;
    const double thd = th * (1.0 + t2 * (g.k[0] + t2 * (g.k[1] + t2 * (g.k[2] + t2 * g.k[3]))));
    const double s = r > 0.0 ? thd / r : 1.0;
    xd = xn * s;
    yd = yn * s;
  }
  u = g.fx * xd + g.cx;
  v = g.fy * yd + g.cy;
  return r2 <= g.r2_max && u >= -0.5 && u <= g.u_hi && v >= -0.5 && v <= g.v_hi;      // every comparison is false for NaN
}

// The one image kernel, for every sampler and pixel layout.  The kernel owns the work split, the pad and the stores; a sampler fills val[j][BGR]
// for those of the 4 pixels (x0 + j, y) of frame `s` that show the frame, and the lens sampler says in in[j] which do (the rest is border; the
// resize has none, so there what is not pad shows the frame and in[] is dead).  The samplers are the two arms of an `if constexpr`, not
// functions: a function, even a forced-inline one, is simplified on its own before it is inlined, and that alone moved the lens kernels by up
// to 4 VGPRs and cost the BGRA one its fifth wave; a computed in[] in the resize arm cost the NV12 one its fifth (94 -> 98 VGPRs).
template <bool LENS, int L, bool VEC>
__global__ __launch_bounds__(256) void image_prep_kernel(const PrepP p, const std::conditional_t<LENS, LensG, ResizeP> sp, const PixSrc f) {
  typedef PixFetch<L> F;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int per_img = p.pad_h * p.qw;
  const long long plane = (long long)p.pad_h * p.pad_w;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += stride) {
    const int img = (int)(idx / per_img);
    const int rem = (int)(idx - (long long)img * per_img);
    const int y = rem / p.qw, x0 = (rem - y * p.qw) * 4;
    float val[4][3];                      // values [x][BGR]
    bool in[4];                           // lens: the pixel shows the frame (the resize has no border: what is not pad shows it)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      in[j] = false;
#pragma unroll
      for (int k = 0; k < 3; ++k) val[j][k] = 0.f;
    }
    if (y < p.dst_h && x0 < p.dst_w) {
      const uint8_t *s = p.src + (long long)img * p.src_image_bytes;
      if constexpr (LENS) {               // ---- lens sampler: G in fp64, four taps, fp32 blend
        const LensG &g = sp;
        const double py = centre(y, g.scale_y);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          double u, v;
          in[j] = x0 + j < p.dst_w && lens_map(g, centre(x0 + j, g.scale_x), py, u, v);
          if (in[j]) {                    // -0.5 <= u <= src_w - 0.5: floor(u) in -1 .. src_w - 1, both taps clamped into the frame
            const double fu_d = floor(u), fv_d = floor(v);
            const int iu = (int)fu_d, iv = (int)fv_d;
            const float fu = (float)(u - fu_d), fv = (float)(v - fv_d);
            const int xa = max(iu, 0), xb = min(iu + 1, g.src_w - 1), ya = max(iv, 0), yb = min(iv + 1, g.src_h - 1);
            int ta[3], tb[3], tc[3], td[3];
            F::px(f, s, xa, ya, ta);
            F::px(f, s, xb, ya, tb);
            F::px(f, s, xa, yb, tc);
            F::px(f, s, xb, yb, td);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              const float a = (float)ta[k], b = (float)tb[k], cc = (float)tc[k], d = (float)td[k];
              const float top = __fadd_rn(a, __fmul_rn(fu, __fsub_rn(b, a)));
              const float bot = __fadd_rn(cc, __fmul_rn(fu, __fsub_rn(d, cc)));
              val[j][k] = __fadd_rn(top, __fmul_rn(fv, __fsub_rn(bot, top)));
            }
          }
        }
      } else {                            // ---- resize sampler: integer copy, exact-half mean or linear resize; 0 .. 255 are exact in fp32
        int v[4][3];                      // resized uint8 values [x][BGR]
        if (sp.mode == PREP_COPY) {                                 // columns past dst_w - 1 are clamped by pair() and discarded below
          F::pair(f, s, x0, y, v[0], v[1]);
          F::pair(f, s, x0 + 2, y, v[2], v[3]);
        } else if (sp.mode == PREP_AREA2) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int x = 2 * min(x0 + j, p.dst_w - 1);             // src_w == 2 * dst_w: both columns exist
            int a[3], b[3], c[3], d[3];
            F::pair(f, s, x, 2 * y, a, b);
            F::pair(f, s, x, 2 * y + 1, c, d);
#pragma unroll
            for (int k = 0; k < 3; ++k) v[j][k] = (a[k] + b[k] + c[k] + d[k] + 2) >> 2;
          }
        } else {
          int sy0, sy1, b0, b1;
          linear_coef(y, sp.scale_y, f.src_h, sy0, sy1, b0, b1);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            int sx0, sx1, a0, a1;
            linear_coef(min(x0 + j, p.dst_w - 1), sp.scale_x, f.src_w, sx0, sx1, a0, a1);
            int t00[3], t01[3], t10[3], t11[3];
            F::px(f, s, sx0, sy0, t00);
            F::px(f, s, sx1, sy0, t01);
            F::px(f, s, sx0, sy1, t10);
            F::px(f, s, sx1, sy1, t11);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              const int d0 = t00[k] * a0 + t01[k] * a1;                  // <= 255 * 2048
              const int d1 = t10[k] * a0 + t11[k] * a1;
              const int q = (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2;
              v[j][k] = min(max(q, 0), 255);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int k = 0; k < 3; ++k) val[j][k] = (float)v[j][k];
      }
    }
    float *o = p.out + (long long)img * 3 * plane + (long long)y * p.pad_w + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float m = p.mean[c], sd = p.std[c];
      f32x4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool show = LENS ? in[j] : y < p.dst_h && x0 + j < p.dst_w;
        r[j] = show ? __fsub_rn(p.swap ? val[j][2 - c] : val[j][c], m) / sd : 0.f;
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

__global__ __launch_bounds__(256) void map_prep_lens_kernel(const LensMapP p) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int per_map = p.fh * p.fw;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += stride) {
    const int m = (int)(idx / per_map);
    const int rem = (int)(idx - (long long)m * per_map);
    const int i = rem / p.fw, j = rem - i * p.fw;
    const int y = i * p.stride, x = j * p.stride;       // < pad <= 32768: no overflow (i < ceil(pad_h / stride))
    float r = 0.f;
    double u, v;
    if (y < p.dst_h && x < p.dst_w && lens_map(p.g, centre(x, p.g.scale_x), centre(y, p.g.scale_y), u, v)) {
      if (p.src == nullptr) {
        r = 1.0f;
      } else {
        const int sx = min(max((int)floor(u + 0.5), 0), p.g.src_w - 1), sy = min(max((int)floor(v + 0.5), 0), p.g.src_h - 1);
        const uint8_t *row = p.src + (long long)m * p.map_bytes + (long long)sy * p.row_bytes;
        const float val = p.u16 ? (float)reinterpret_cast<const uint16_t *>(row)[sx] : reinterpret_cast<const float *>(row)[sx];
        r = __fmul_rn(p.scale, val);
      }
    }
    p.out[idx] = r;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host: the checks
// The checks of an ivx_image_prep_desc that every entry makes, with one text (what: the entry's name): the size rules (the map entry stops
// here) ...
int prep_check_sizes(const ivx_image_prep_desc *d, const int32_t n, const char *what) {
  IVX_REQUIRE(d->src_h > 0 && d->src_w > 0 && d->dst_h > 0 && d->dst_w > 0, "%s: sizes must be positive (src %d x %d, dst %d x %d)", what, d->src_h,
              d->src_w, d->dst_h, d->dst_w);
  IVX_REQUIRE(d->pad_h >= d->dst_h && d->pad_w >= d->dst_w, "%s: pad %d x %d is smaller than dst %d x %d", what, d->pad_h, d->pad_w, d->dst_h,
              d->dst_w);
  IVX_REQUIRE(d->src_h <= kPrepMaxDim && d->src_w <= kPrepMaxDim && d->pad_h <= kPrepMaxDim && d->pad_w <= kPrepMaxDim,
              "%s: extents above %d are not supported (src %d x %d, pad %d x %d)", what, kPrepMaxDim, d->src_h, d->src_w, d->pad_h, d->pad_w);
  IVX_REQUIRE(n > 0 && n <= kPrepMaxFrames, "%s: n = %d must be in 1 .. %d", what, n, kPrepMaxFrames);
  return IVX_OK;
}
// ... and, for the image entries, the pitch of plane 0 against the layout's bound and the normalisation (sizes checked before)
int prep_check_rows(const ivx_image_prep_desc *d, const int layout, const char *what) {
  const int64_t w = d->src_w, cw = (w + 1) / 2;
  static const char *const rule[IVX_PIX_COUNT] = {"3 * src_w", "3 * src_w", "4 * src_w", "4 * src_w", "src_w", "src_w", "4 * ceil(src_w / 2)"};
  const int64_t need[IVX_PIX_COUNT] = {3 * w, 3 * w, 4 * w, 4 * w, w, w, 4 * cw};
  IVX_REQUIRE((int64_t)d->src_row_bytes >= need[layout], "%s: src_row_bytes %d is below %s = %lld", what, d->src_row_bytes, rule[layout],
              (long long)need[layout]);
  for (int c = 0; c < 3; ++c) IVX_REQUIRE(isfinite(d->std[c]) && d->std[c] != 0.f, "%s: std[%d] = %g must be finite and non-zero", what, c, (double)d->std[c]);
  return IVX_OK;
}

// packed BGR as the entries before 0.5.3 take it: no second plane, no matrix, byte loads
PixSrc pix_src_bgr8(const ivx_image_prep_desc *d) {
  PixSrc s = {};
  s.src_h = d->src_h, s.src_w = d->src_w, s.row_bytes = d->src_row_bytes;
  return s;
}

// the fmt entry's checks of a frame format (layout and row pitch checked before) and of the source geometry that depends on it; fills `s`
int pix_src_fill(PixSrc &s, const ivx_image_prep_desc *d, const ivx_frame_format *f, const void *src, const int64_t src_image_bytes, const int32_t n,
                 const char *what) {
  const int64_t w = d->src_w, cw = (w + 1) / 2, ch = ((int64_t)d->src_h + 1) / 2;
  int64_t last = (int64_t)d->src_h * d->src_row_bytes;         // one past the last byte of the last plane
  s.plane1_offset = 0;
  s.plane1_row_bytes = 0;
  if (f->layout == IVX_PIX_NV12) {
    IVX_REQUIRE((int64_t)f->plane1_row_bytes >= 2 * cw, "%s: plane1_row_bytes %d is below 2 * ceil(src_w / 2) = %lld", what, f->plane1_row_bytes,
                (long long)(2 * cw));
    IVX_REQUIRE(f->plane1_offset >= last, "%s: plane1_offset %lld is below src_h * src_row_bytes = %lld", what, (long long)f->plane1_offset,
                (long long)last);
    IVX_REQUIRE(f->plane1_offset <= ((int64_t)1 << 46), "%s: plane1_offset %lld is above 2^46", what, (long long)f->plane1_offset);
    s.plane1_offset = f->plane1_offset;
    s.plane1_row_bytes = f->plane1_row_bytes;
    last = f->plane1_offset + ch * f->plane1_row_bytes;
  }
  const bool yuv = f->layout == IVX_PIX_NV12 || f->layout == IVX_PIX_YUYV;
  if (yuv) {
    IVX_REQUIRE(f->y_off >= 0 && f->y_off <= 255, "%s: y_off = %d must be in 0 .. 255", what, f->y_off);
    const int32_t c[5] = {f->cy, f->cub, f->cug, f->cvg, f->cvr};
    static const char *const cn[5] = {"cy", "cub", "cug", "cvg", "cvr"};
    for (int i = 0; i < 5; ++i)
      IVX_REQUIRE(c[i] >= -IVX_YUV_COEF_MAX && c[i] <= IVX_YUV_COEF_MAX, "%s: coefficient %s = %d is outside +-(3 << 20) = +-%d", what, cn[i], c[i],
                  IVX_YUV_COEF_MAX);
  }
  IVX_REQUIRE(n == 1 || src_image_bytes >= last, "%s: src_image_bytes %lld does not cover the last plane, which ends at byte %lld", what,
              (long long)src_image_bytes, (long long)last);
  s.src_h = d->src_h, s.src_w = d->src_w, s.row_bytes = d->src_row_bytes;
  s.y_off = yuv ? f->y_off : 0;
  s.cy = yuv ? f->cy : 0, s.cub = yuv ? f->cub : 0, s.cug = yuv ? f->cug : 0, s.cvg = yuv ? f->cvg : 0, s.cvr = yuv ? f->cvr : 0;
  const uintptr_t base = (uintptr_t)src;
  const int64_t step = n == 1 ? 0 : src_image_bytes;
  if (f->layout == IVX_PIX_NV12) s.wide = ((base + (uintptr_t)f->plane1_offset) % 2 == 0) && f->plane1_row_bytes % 2 == 0 && step % 2 == 0;
  else if (f->layout == IVX_PIX_YUYV || f->layout == IVX_PIX_BGRA8 || f->layout == IVX_PIX_RGBA8)
    s.wide = base % 4 == 0 && d->src_row_bytes % 4 == 0 && step % 4 == 0;
  else s.wide = 0;
  return IVX_OK;
}

bool finite_nz(const double v) { return isfinite(v) && v != 0.0; }

int check_lens(const ivx_lens *l, const char *what) {
  IVX_REQUIRE(l->model == IVX_LENS_BROWN || l->model == IVX_LENS_FISHEYE, "%s: unknown lens model %d (IVX_LENS_BROWN = 0, IVX_LENS_FISHEYE = 1)", what,
              l->model);
  IVX_REQUIRE(finite_nz(l->fx) && finite_nz(l->fy) && finite_nz(l->new_fx) && finite_nz(l->new_fy),
              "%s: focal lengths must be finite and non-zero (fx %g, fy %g, new_fx %g, new_fy %g)", what, l->fx, l->fy, l->new_fx, l->new_fy);
  IVX_REQUIRE(isfinite(l->cx) && isfinite(l->cy) && isfinite(l->new_cx) && isfinite(l->new_cy),
              "%s: principal points must be finite (cx %g, cy %g, new_cx %g, new_cy %g)", what, l->cx, l->cy, l->new_cx, l->new_cy);
  for (int i = 0; i < 5; ++i) IVX_REQUIRE(isfinite(l->coef[i]), "%s: coef[%d] = %g must be finite", what, i, l->coef[i]);
  IVX_REQUIRE(l->r2_max > 0.0, "%s: r2_max = %g must be > 0 or +inf", what, l->r2_max);      // (NaN fails the comparison)
  return IVX_OK;
}

// ------------------------------------------------------------------------------------------------------- host: parameters and launch
void fill_geometry(LensG &g, const ivx_image_prep_desc *d, const ivx_lens *l) {
  g.model = l ? l->model : -1;
  g.src_h = d->src_h, g.src_w = d->src_w;
  g.scale_x = (double)d->src_w / (double)d->dst_w;
  g.scale_y = (double)d->src_h / (double)d->dst_h;
  g.u_hi = (double)d->src_w - 0.5, g.v_hi = (double)d->src_h - 0.5;
  g.fx = g.fy = g.nfx = g.nfy = 1.0;
  g.cx = g.cy = g.ncx = g.ncy = 0.0;
  for (int i = 0; i < 5; ++i) g.k[i] = 0.0;
  g.r2_max = INFINITY;
  if (l) {
    g.fx = l->fx, g.fy = l->fy, g.cx = l->cx, g.cy = l->cy;
    g.nfx = l->new_fx, g.nfy = l->new_fy, g.ncx = l->new_cx, g.ncy = l->new_cy;
    for (int i = 0; i < 5; ++i) g.k[i] = l->coef[i];
    g.r2_max = l->r2_max;
  }
}

// the skeleton's record from a checked call
PrepP prep_fill(const ivx_image_prep_desc *d, const void *src, const int64_t src_image_bytes, const int32_t n, float *out) {
  PrepP p;
  p.src = (const uint8_t *)src;
  p.out = out;
  p.src_image_bytes = n == 1 ? 0 : src_image_bytes;
  p.dst_h = d->dst_h, p.dst_w = d->dst_w, p.pad_h = d->pad_h, p.pad_w = d->pad_w;
  p.qw = (d->pad_w + 3) / 4;
  p.total = (long long)n * d->pad_h * p.qw;
  p.swap = d->to_rgb != 0;
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = d->mean[c];
    p.std[c] = d->std[c];
  }
  return p;
}

// the capped grid of `total` work items, and whether rows of row_w floats at `out` take 16-byte stores
struct PrepGrid {
  unsigned blocks;
  bool vec;
};
PrepGrid prep_grid(const long long total, const float *out, const int row_w) {
  long long blocks = (total + 255) / 256;
  if (blocks > kPrepGridCap) blocks = kPrepGridCap;
  return {(unsigned)blocks, row_w % 4 == 0 && ((uintptr_t)out & 15) == 0};
}

template <bool LENS, int L>
void prep_launch_layout(const PrepGrid &g, ivx_stream_t stream, const PrepP &p, const std::conditional_t<LENS, LensG, ResizeP> &sp, const PixSrc &f) {
  if (g.vec) hipLaunchKernelGGL((image_prep_kernel<LENS, L, true>), dim3(g.blocks), dim3(256), 0, (hipStream_t)stream, p, sp, f);
  else hipLaunchKernelGGL((image_prep_kernel<LENS, L, false>), dim3(g.blocks), dim3(256), 0, (hipStream_t)stream, p, sp, f);
}

// Check the lens (nullptr: none), fill the kernel's parameters from the CHECKED d / f / n and launch the layout's instantiation.
// what: the calling entry's name.
int prep_launch(const ivx_image_prep_desc *d, const int32_t layout, const PixSrc &f, const ivx_lens *lens, const void *src, const int64_t src_image_bytes,
                const int32_t n, float *out, ivx_stream_t stream, const char *what) {
  if (lens)
    if (int e = check_lens(lens, what)) return e;
  const PrepP p = prep_fill(d, src, src_image_bytes, n, out);
  const PrepGrid g = prep_grid(p.total, out, d->pad_w);
  LensG lg;
  fill_geometry(lg, d, lens);
  ResizeP r;
  r.scale_x = lg.scale_x, r.scale_y = lg.scale_y;
  // the order of data.imresize_cv2_linear: equal size is a copy, an exact half on BOTH axes the INTER_AREA mean, the tables otherwise
  r.mode = (d->src_h == d->dst_h && d->src_w == d->dst_w)           ? PREP_COPY
           : (d->src_h == 2 * d->dst_h && d->src_w == 2 * d->dst_w) ? PREP_AREA2
                                                                    : PREP_LINEAR;
#define IVX_PREP_LAUNCH(L)                                              \
  if (lens) prep_launch_layout<true, L>(g, stream, p, lg, f);   \
  else prep_launch_layout<false, L>(g, stream, p, r, f)
  IVX_PIX_DISPATCH(layout, IVX_PREP_LAUNCH)
#undef IVX_PREP_LAUNCH
  IVX_CHECK_LAUNCH(what);
  return IVX_OK;
}

// The one checked path of the three image entries (null pointers are the entry's own check).  fmt == nullptr: packed BGR as the entries
// before 0.5.3 take it, with their src_image_bytes rule.
int image_prep(const char *what, const ivx_image_prep_desc *d, const ivx_frame_format *fmt, const ivx_lens *lens, const void *src,
               const int64_t src_image_bytes, const int32_t n, float *out, ivx_stream_t stream) {
  const int32_t layout = fmt ? fmt->layout : IVX_PIX_BGR8;
  if (int e = prep_check_sizes(d, n, what)) return e;
  if (int e = prep_check_rows(d, layout, what)) return e;
  PixSrc f = pix_src_bgr8(d);
  if (fmt) {
    if (int e = pix_src_fill(f, d, fmt, src, src_image_bytes, n, what)) return e;
  } else {
    IVX_REQUIRE(n == 1 || src_image_bytes >= (int64_t)d->src_h * d->src_row_bytes, "%s: src_image_bytes %lld is below src_h * src_row_bytes = %lld", what,
                (long long)src_image_bytes, (long long)d->src_h * d->src_row_bytes);
  }
  return prep_launch(d, layout, f, lens, src, src_image_bytes, n, out, stream, what);
}

// num / den (den > 0) rounded half to even, in integers
int64_t div_half_even(const int64_t num, const int64_t den) {
  int64_t q = num / den, r = num % den;
  if (r < 0) { q -= 1; r += den; }                  // floor
  if (2 * r > den || (2 * r == den && (q & 1))) q += 1;
  return q;
}

}  // namespace

extern "C" int ivx_image_prep_u8(const ivx_image_prep_desc *d, const void *src, int64_t src_image_bytes, int32_t n, float *out,
                                 ivx_stream_t stream) {
  IVX_REQUIRE(d && src && out, "ivx_image_prep_u8: null argument");
  return image_prep("ivx_image_prep_u8", d, nullptr, nullptr, src, src_image_bytes, n, out, stream);
}

extern "C" int ivx_image_prep_lens_u8(const ivx_image_prep_desc *d, const ivx_lens *lens, const void *src, int64_t src_image_bytes, int32_t n,
                                      float *out, ivx_stream_t stream) {
  IVX_REQUIRE(d && lens && src && out, "ivx_image_prep_lens_u8: null argument");
  return image_prep("ivx_image_prep_lens_u8", d, nullptr, lens, src, src_image_bytes, n, out, stream);
}

extern "C" int ivx_image_prep_fmt_u8(const ivx_image_prep_desc *d, const ivx_frame_format *fmt, const ivx_lens *lens, const void *src,
                                     int64_t src_image_bytes, int32_t n, float *out, ivx_stream_t stream) {
  IVX_REQUIRE(d && src && out, "ivx_image_prep_fmt_u8: null argument");
  IVX_REQUIRE(fmt, "ivx_image_prep_fmt_u8: null frame format");
  IVX_REQUIRE(fmt->layout >= 0 && fmt->layout < IVX_PIX_COUNT, "ivx_image_prep_fmt_u8: unknown layout %d (IVX_PIX_BGR8 = 0 .. IVX_PIX_YUYV = 6)", fmt->layout);
  return image_prep("ivx_image_prep_fmt_u8", d, fmt, lens, src, src_image_bytes, n, out, stream);
}

extern "C" int ivx_map_prep_lens(const ivx_image_prep_desc *d, const ivx_lens *lens, const void *src, int32_t src_dtype, int64_t src_row_bytes,
                                 int64_t src_map_bytes, float scale, int32_t stride, int32_t n, float *out, ivx_stream_t stream) {
  static const char *const what = "ivx_map_prep_lens";
  IVX_REQUIRE(d && out, "ivx_map_prep_lens: null argument");
  if (int e = prep_check_sizes(d, n, what)) return e;
  IVX_REQUIRE(stride >= 1, "ivx_map_prep_lens: stride = %d must be >= 1", stride);
  if (lens)
    if (int e = check_lens(lens, what)) return e;
  LensMapP p;
  fill_geometry(p.g, d, lens);
  p.src = (const uint8_t *)src;
  p.out = out;
  p.row_bytes = p.map_bytes = 0;
  p.u16 = 0;
  p.scale = 1.0f;
  if (src) {
    IVX_REQUIRE(src_dtype == IVX_MAP_F32 || src_dtype == IVX_MAP_U16, "ivx_map_prep_lens: unknown src_dtype %d (IVX_MAP_F32 = 0, IVX_MAP_U16 = 1)",
                src_dtype);
    const int64_t es = src_dtype == IVX_MAP_U16 ? 2 : 4;
    IVX_REQUIRE(src_row_bytes >= es * (int64_t)d->src_w && src_row_bytes % es == 0,
                "ivx_map_prep_lens: src_row_bytes %lld must be a multiple of %lld and at least %lld * src_w = %lld", (long long)src_row_bytes,
                (long long)es, (long long)es, (long long)(es * d->src_w));
    IVX_REQUIRE(((uintptr_t)src % es) == 0, "ivx_map_prep_lens: src is not aligned to its %lld-byte elements", (long long)es);
    IVX_REQUIRE(n == 1 || (src_map_bytes >= (int64_t)d->src_h * src_row_bytes && src_map_bytes % es == 0),
                "ivx_map_prep_lens: src_map_bytes %lld must be a multiple of %lld and at least src_h * src_row_bytes = %lld", (long long)src_map_bytes,
                (long long)es, (long long)d->src_h * (long long)src_row_bytes);
    IVX_REQUIRE(isfinite(scale), "ivx_map_prep_lens: scale = %g must be finite", (double)scale);
    p.row_bytes = src_row_bytes;
    p.map_bytes = n == 1 ? 0 : src_map_bytes;
    p.u16 = src_dtype == IVX_MAP_U16;
    p.scale = scale;
  }
  p.dst_h = d->dst_h, p.dst_w = d->dst_w;
  p.stride = stride;
  p.fh = (d->pad_h - 1) / stride + 1, p.fw = (d->pad_w - 1) / stride + 1;      // ceil(pad / stride) without overflow at a large stride
  p.total = (long long)n * p.fh * p.fw;
  hipLaunchKernelGGL(map_prep_lens_kernel, dim3(prep_grid(p.total, out, p.fw).blocks), dim3(256), 0, (hipStream_t)stream, p);
  IVX_CHECK_LAUNCH("ivx_map_prep_lens");
  return IVX_OK;
}

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
