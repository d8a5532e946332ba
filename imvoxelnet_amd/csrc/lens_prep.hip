// Lens-aware device image pipeline (include/imvoxel.h, ivx_image_prep_lens_u8 / ivx_map_prep_lens): uint8 HWC BGR frames of a real camera
// -> Undistort -> Resize -> Normalize -> Pad as ONE launch, and the cover / depth maps of the same geometry at feature resolution.
//
// One geometric map G (the header writes every step) takes a pixel of the network input back to the raw frame: the resize's pixel-centre
// rule, the ideal camera new_K backwards, the distortion polynomial (OpenCV's 5-coefficient Brown model or its equidistant fisheye model)
// forwards, the real camera K.  G is evaluated once per pixel in fp64, each operation rounded on its own (this file is built with
// -ffp-contract=off, and the host reference restates the same order), so the coordinates of the kernel and of an fp64 reference agree to
// a few ulp of fp64 and every decision (inside / border, which four taps, which nearest pixel) can be made robust by the reference alone.
// The blend after it is fp32 in the header's order; the fractions are rounded once.
//
// Image kernel: the work split of csrc/preprocess.hip -- one thread produces 4 consecutive output x of one output row for all three planes
// (three 16-byte stores; scalar stores when pad_w % 4 != 0 or `out` is not 16-byte aligned), items numbered x fastest, then y, then frame,
// capped grid with a grid-stride loop.  The gather reads 2 x 2 x 3 bytes per pixel; neighbouring lanes map to neighbouring source pixels
// (G is smooth), so a wavefront's taps fall into a few source rows and the cache lines are shared as in the plain kernel.
// Map kernel: one lane per feature pixel; tiny and launch-bound.  No LDS, no atomics, plain vector stores.
#include "ivx_common.h"
#include "pixel_fetch.h"

#include <math.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct LensG {                           // what G needs: the lens (model < 0: the ideal camera) and the resize
  int model;
  int src_h, src_w;
  double scale_x, scale_y;               // double(src) / double(dst)
  double fx, fy, cx, cy, k[5], nfx, nfy, ncx, ncy, r2_max;
  double u_hi, v_hi;                     // src_w - 0.5, src_h - 0.5
};

struct LensPrepP {
  LensG g;
  const uint8_t *src;
  float *out;
  long long src_image_bytes, total;      // total = n * pad_h * qw work items
  int dst_h, dst_w, pad_h, pad_w, qw;       // (the source geometry is PixSrc's)
  int swap;                              // to_rgb: output channel c reads source channel 2 - c
  float mean[3], std[3];
};

struct LensMapP {
  LensG g;
  const uint8_t *src;                    // nullptr: the cover map
  float *out;
  long long row_bytes, map_bytes, total; // total = n * fh * fw
  int dst_h, dst_w, fh, fw, stride, u16;
  float scale;
};

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

// The image kernel, for every pixel layout (0.5.3): the four taps are fetched through a policy of pixel_fetch.h -- each tap is fetched (and, for
// the YUV layouts, converted to its three BGR bytes) once -- and blended in fp32 in the header's order.  ivx_image_prep_lens_u8 launches the
// BGR8 instantiation (same bits as the kernel it had before, tests/golden/image_prep_bgr_0_5_2.npz; 0.79 .. 0.89 of its time).
template <int L, bool VEC>
__global__ __launch_bounds__(256) void image_prep_fmt_lens_u8_kernel(const LensPrepP p, const PixSrc f) {
  typedef PixFetch<L> F;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int per_img = p.pad_h * p.qw;
  const long long plane = (long long)p.pad_h * p.pad_w;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += stride) {
    const int img = (int)(idx / per_img);
    const int rem = (int)(idx - (long long)img * per_img);
    const int y = rem / p.qw, x0 = (rem - y * p.qw) * 4;
    float val[4][3];                      // blended values [x][BGR]
    bool in[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      in[j] = false;
#pragma unroll
      for (int k = 0; k < 3; ++k) val[j][k] = 0.f;
    }
    if (y < p.dst_h && x0 < p.dst_w) {
      const uint8_t *s = p.src + (long long)img * p.src_image_bytes;
      const double py = centre(y, p.g.scale_y);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double u, v;
        in[j] = x0 + j < p.dst_w && lens_map(p.g, centre(x0 + j, p.g.scale_x), py, u, v);
        if (in[j]) {                      // -0.5 <= u <= src_w - 0.5: floor(u) in -1 .. src_w - 1, both taps clamped into the frame
          const double fu_d = floor(u), fv_d = floor(v);
          const int iu = (int)fu_d, iv = (int)fv_d;
          const float fu = (float)(u - fu_d), fv = (float)(v - fv_d);
          const int xa = max(iu, 0), xb = min(iu + 1, p.g.src_w - 1), ya = max(iv, 0), yb = min(iv + 1, p.g.src_h - 1);
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
    }
    float *o = p.out + (long long)img * 3 * plane + (long long)y * p.pad_w + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float m = p.mean[c], sd = p.std[c];
      f32x4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = in[j] ? __fsub_rn(p.swap ? val[j][2 - c] : val[j][c], m) / sd : 0.f;
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

}  // namespace

// Check the lens, fill the kernel's parameters from a checked call and launch the layout's instantiation (declared in pixel_fetch.h)
int ivx_image_prep_lens_launch(const ivx_image_prep_desc *d, int32_t layout, const PixSrc &f, const ivx_lens *lens, const void *src,
                               int64_t src_image_bytes, int32_t n, float *out, ivx_stream_t stream, const char *what) {
  if (int e = check_lens(lens, what)) return e;
  LensPrepP p;
  fill_geometry(p.g, d, lens);
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
  long long blocks = (p.total + 255) / 256;
  if (blocks > kPrepGridCap) blocks = kPrepGridCap;
  const bool vec = d->pad_w % 4 == 0 && ((uintptr_t)out & 15) == 0;
#define IVX_LENS_LAUNCH(L)                                                                                                              \
  if (vec) hipLaunchKernelGGL((image_prep_fmt_lens_u8_kernel<L, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, f); \
  else hipLaunchKernelGGL((image_prep_fmt_lens_u8_kernel<L, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, f)
  IVX_PIX_DISPATCH(layout, IVX_LENS_LAUNCH)
#undef IVX_LENS_LAUNCH
  IVX_CHECK_LAUNCH(what);
  return IVX_OK;
}

extern "C" int ivx_image_prep_lens_u8(const ivx_image_prep_desc *d, const ivx_lens *lens, const void *src, int64_t src_image_bytes, int32_t n,
                                      float *out, ivx_stream_t stream) {
  static const char *const what = "ivx_image_prep_lens_u8";
  IVX_REQUIRE(d && lens && src && out, "ivx_image_prep_lens_u8: null argument");
  if (int e = prep_check_sizes(d, n, what)) return e;
  if (int e = prep_check_rows(d, IVX_PIX_BGR8, what)) return e;
  IVX_REQUIRE(n == 1 || src_image_bytes >= (int64_t)d->src_h * d->src_row_bytes,
              "ivx_image_prep_lens_u8: src_image_bytes %lld is below src_h * src_row_bytes = %lld", (long long)src_image_bytes,
              (long long)d->src_h * d->src_row_bytes);
  return ivx_image_prep_lens_launch(d, IVX_PIX_BGR8, pix_src_bgr8(d), lens, src, src_image_bytes, n, out, stream, what);
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
  long long blocks = (p.total + 255) / 256;
  if (blocks > kPrepGridCap) blocks = kPrepGridCap;
  hipLaunchKernelGGL(map_prep_lens_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  IVX_CHECK_LAUNCH("ivx_map_prep_lens");
  return IVX_OK;
}
