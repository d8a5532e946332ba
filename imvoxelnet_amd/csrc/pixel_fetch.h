// Source access of the device image pipeline for the decoder pixel formats of include/imvoxel.h (0.5.3, ivx_frame_format): ONE place that
// knows how the bytes of a frame lie.  A frame in any layout IS a BGR uint8 frame through the header's integer rule; a fetch policy
// PixFetch<LAYOUT> returns the three bytes of pixel (x, y) in BGR order, and the image kernel of csrc/image_prep.hip and its two samplers are
// templated on it, so the resize, the lens map, the blend, the normalisation and the pad are written once and see BGR bytes only.
//
//   px(f, frame, x, y, bgr)              one pixel (the taps of the linear resize and of the lens gather: arbitrary columns)
//   pair(f, frame, x, y, bgr0, bgr1)     columns min(x, src_w - 1) and min(x + 1, src_w - 1) of row y, x EVEN (the copy and the exact-half
//                                        paths read consecutive columns): for NV12 and YUYV the two share one chroma pair, which is loaded
//                                        and multiplied once
// Loads: the (U, V) pair of NV12 is one 2-byte load, the macropixel of YUYV and the pixel of BGRA / RGBA one 4-byte load, when the host
// has CHECKED that every such address is aligned (PixSrc.wide: base pointer, plane offset, pitches and frame stride all multiples of the
// access size); otherwise byte loads.  Pitch and offset are the caller's: nothing is assumed.  The Y bytes of NV12 and the bytes of the
// 3-byte layouts stay byte loads (a wave's lanes read neighbouring bytes of the same cache lines).  Measured, the kernels are not bound by
// memory: the needed bytes move at 1.1 .. 2.3 TB/s for the YUV layouts and the time follows the integer work per tap
// (profiles/image_prep_fmt.md; a reading from rates and instruction counts, no counter run was made).
// The conversion is plain int32 C++: with |coefficient| <= 3 << 20 and 0 <= y_off <= 255 no intermediate leaves int32
// (255 * 3 * 2^20 + 2 * 128 * 3 * 2^20 + 2^19 < 2^31); `>>` on a negative int is an arithmetic shift on this target, the floor the header asks for.
#pragma once
#include "ivx_common.h"

#define IVX_PIX_COUNT 7
#define IVX_YUV_COEF_MAX (3 << 20)

struct PixSrc {                          // how the source frames lie (filled and checked on the host by csrc/image_prep.hip pix_src_fill)
  long long plane1_offset;               // NV12: bytes from a frame's first byte to its UV plane
  int src_h, src_w, row_bytes, plane1_row_bytes;
  int y_off, cy, cub, cug, cvg, cvr;     // YUV layouts: the integer matrix, 20 fractional bits
  int wide;                              // the 2- / 4-byte loads of the layout are aligned (checked on the host)
};

#if defined(__HIPCC__)
__device__ __forceinline__ int pix_clamp(const int v) { return min(max(v, 0), 255); }

// the chroma terms of the header's rule, shared by the pixels of one (U, V) pair: (B, G, R) additions before the shift
__device__ __forceinline__ void pix_chroma(const PixSrc &f, const int U, const int V, int c[3]) {
  const int u = U - 128, v = V - 128;
  c[0] = f.cub * u;
  c[1] = f.cvg * v + f.cug * u;
  c[2] = f.cvr * v;
}
__device__ __forceinline__ void pix_yuv(const PixSrc &f, const int Y, const int c[3], int bgr[3]) {
  const int yy = max(0, Y - f.y_off) * f.cy + (1 << 19);
#pragma unroll
  for (int k = 0; k < 3; ++k) bgr[k] = pix_clamp((yy + c[k]) >> 20);
}

template <int L>
struct PixFetch;

// the layouts without shared samples: pair() is px() twice
template <int L>
struct PixFetchPlain {
  static __device__ __forceinline__ void pair(const PixSrc &f, const uint8_t *s, const int x, const int y, int a[3], int b[3]) {
    PixFetch<L>::px(f, s, min(x, f.src_w - 1), y, a);
    PixFetch<L>::px(f, s, min(x + 1, f.src_w - 1), y, b);
  }
};

template <>
struct PixFetch<IVX_PIX_BGR8> : PixFetchPlain<IVX_PIX_BGR8> {
  static __device__ __forceinline__ void px(const PixSrc &f, const uint8_t *s, const int x, const int y, int bgr[3]) {
    const uint8_t *p = s + (long long)y * f.row_bytes + 3 * x;
    bgr[0] = p[0], bgr[1] = p[1], bgr[2] = p[2];
  }
};
template <>
struct PixFetch<IVX_PIX_RGB8> : PixFetchPlain<IVX_PIX_RGB8> {
  static __device__ __forceinline__ void px(const PixSrc &f, const uint8_t *s, const int x, const int y, int bgr[3]) {
    const uint8_t *p = s + (long long)y * f.row_bytes + 3 * x;
    bgr[0] = p[2], bgr[1] = p[1], bgr[2] = p[0];
  }
};
// the 4-byte pixel, byte 3 ignored: (c0, c1, c2) in memory order
__device__ __forceinline__ void pix_load4(const PixSrc &f, const uint8_t *p, int &c0, int &c1, int &c2) {
  if (f.wide) {
    const uint32_t w = *reinterpret_cast<const uint32_t *>(p);
    c0 = w & 255, c1 = (w >> 8) & 255, c2 = (w >> 16) & 255;
  } else {
    c0 = p[0], c1 = p[1], c2 = p[2];
  }
}
template <>
struct PixFetch<IVX_PIX_BGRA8> : PixFetchPlain<IVX_PIX_BGRA8> {
  static __device__ __forceinline__ void px(const PixSrc &f, const uint8_t *s, const int x, const int y, int bgr[3]) {
    pix_load4(f, s + (long long)y * f.row_bytes + 4 * x, bgr[0], bgr[1], bgr[2]);
  }
};
template <>
struct PixFetch<IVX_PIX_RGBA8> : PixFetchPlain<IVX_PIX_RGBA8> {
  static __device__ __forceinline__ void px(const PixSrc &f, const uint8_t *s, const int x, const int y, int bgr[3]) {
    pix_load4(f, s + (long long)y * f.row_bytes + 4 * x, bgr[2], bgr[1], bgr[0]);
  }
};
template <>
struct PixFetch<IVX_PIX_GRAY8> : PixFetchPlain<IVX_PIX_GRAY8> {
  static __device__ __forceinline__ void px(const PixSrc &f, const uint8_t *s, const int x, const int y, int bgr[3]) {
    bgr[0] = bgr[1] = bgr[2] = s[(long long)y * f.row_bytes + x];
  }
};

template <>
struct PixFetch<IVX_PIX_NV12> {
  // the (U, V) pair of pixel (x, y): [y >> 1][x >> 1] of plane 1
  static __device__ __forceinline__ void chroma(const PixSrc &f, const uint8_t *s, const int x, const int y, int c[3]) {
    const uint8_t *p = s + f.plane1_offset + (long long)(y >> 1) * f.plane1_row_bytes + 2 * (x >> 1);
    int U, V;
    if (f.wide) {
      const uint32_t w = *reinterpret_cast<const uint16_t *>(p);
      U = w & 255, V = w >> 8;
    } else {
      U = p[0], V = p[1];
    }
    pix_chroma(f, U, V, c);
  }
  static __device__ __forceinline__ void px(const PixSrc &f, const uint8_t *s, const int x, const int y, int bgr[3]) {
    int c[3];
    chroma(f, s, x, y, c);
    pix_yuv(f, s[(long long)y * f.row_bytes + x], c, bgr);
  }
  static __device__ __forceinline__ void pair(const PixSrc &f, const uint8_t *s, const int x, const int y, int a[3], int b[3]) {
    const int xa = min(x, f.src_w - 1), xb = min(x + 1, f.src_w - 1);      // x even: xa >> 1 == xb >> 1
    int c[3];
    chroma(f, s, xa, y, c);
    const uint8_t *r = s + (long long)y * f.row_bytes;
    pix_yuv(f, r[xa], c, a);
    pix_yuv(f, r[xb], c, b);
  }
};

template <>
struct PixFetch<IVX_PIX_YUYV> {
  // macropixel x >> 1 of row y: (Y0, U, Y1, V)
  static __device__ __forceinline__ void macro(const PixSrc &f, const uint8_t *s, const int x, const int y, int &Y0, int &Y1, int c[3]) {
    const uint8_t *p = s + (long long)y * f.row_bytes + 4 * (x >> 1);
    int U, V;
    if (f.wide) {
      const uint32_t w = *reinterpret_cast<const uint32_t *>(p);
      Y0 = w & 255, U = (w >> 8) & 255, Y1 = (w >> 16) & 255, V = w >> 24;
    } else {
      Y0 = p[0], U = p[1], Y1 = p[2], V = p[3];
    }
    pix_chroma(f, U, V, c);
  }
  static __device__ __forceinline__ void px(const PixSrc &f, const uint8_t *s, const int x, const int y, int bgr[3]) {
    int Y0, Y1, c[3];
    macro(f, s, x, y, Y0, Y1, c);
    pix_yuv(f, (x & 1) ? Y1 : Y0, c, bgr);
  }
  static __device__ __forceinline__ void pair(const PixSrc &f, const uint8_t *s, const int x, const int y, int a[3], int b[3]) {
    const int xa = min(x, f.src_w - 1), xb = min(x + 1, f.src_w - 1);      // x even: one macropixel
    int Y0, Y1, c[3];
    macro(f, s, xa, y, Y0, Y1, c);
    pix_yuv(f, (xa & 1) ? Y1 : Y0, c, a);
    pix_yuv(f, (xb & 1) ? Y1 : Y0, c, b);
  }
};

// LAUNCH(L) for the checked layout
#define IVX_PIX_DISPATCH(layout, LAUNCH)                  \
  switch (layout) {                                       \
    case IVX_PIX_BGR8: LAUNCH(IVX_PIX_BGR8); break;       \
    case IVX_PIX_RGB8: LAUNCH(IVX_PIX_RGB8); break;       \
    case IVX_PIX_BGRA8: LAUNCH(IVX_PIX_BGRA8); break;     \
    case IVX_PIX_RGBA8: LAUNCH(IVX_PIX_RGBA8); break;     \
    case IVX_PIX_GRAY8: LAUNCH(IVX_PIX_GRAY8); break;     \
    case IVX_PIX_NV12: LAUNCH(IVX_PIX_NV12); break;       \
    default: LAUNCH(IVX_PIX_YUYV); break;                 \
  }
#endif
