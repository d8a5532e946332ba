// The geometry chain of the image-to-voxel lift, written once as device functions: the voxel of an index, its centre, the projection of a
// centre by one view's rows, the validity rule, and the two tests the pixel maps add (include/imvoxel.h: ivx_backproject_mean_fwd,
// ivx_backproject_mapped_fwd step 3).
//
// Who uses it.  Both lift kernels of csrc/backproject.hip and the coverage kernel of csrc/view_coverage.hip (ivx_view_coverage_fwd): nothing
// else in csrc/ splits a voxel index, projects a centre or decides validity.  csrc/volume_warp.hip (ivx_volume_warp_fwd) takes the voxel of an
// index, its centre and the row product from here for its rigid transform (no projection, no validity).  tests/test_gpu_view_coverage.py still checks on the device that
// the coverage count of a view equals the lift's mask of that view: it guards the two callers (their crop, slot and map addressing), not two texts.
// profiles/lift_one_geometry.md compares the code the lift kernels compile to with what their inline chain compiled to.
//
// Arithmetic.  Every operation is fp32, round-to-nearest, and spelled with the __f*_rn intrinsics, so no product and sum is ever contracted
// whatever the flags of the including file (which is compiled with -ffp-contract=off all the same):
//   point   = float(idx) * voxel_size + new_origin                 (a product, a sum)
//   (u,v,d) = fma(P3, 1, fma(P2, z, fma(P1, y, P0 * x)))           per row of P [3,4]  (what torch.bmm does on CPU)
//   xf, yf  = u / d, v / d                                          (IEEE division)
//   xr, yr  = rint(xf), rint(yf)                                    (round-half-even)
//   valid   = 0 <= xr < wc && 0 <= yr < hc && d > 0                 (on the rounded floats: NaN and inf fail, as do the INT64_MIN values the
//                                                                    reference's .long() produces for them)
// P may be a uniform address (a slot's rows): the loads then go through the scalar cache and the twelve numbers live in scalar registers.
#pragma once
#include <hip/hip_runtime.h>

// The voxel of a flat index: n = (i * Y + j) * Z + k.
template <typename I>
__device__ __forceinline__ void lift_voxel(const I n, const int Y, const int Z, int &i, int &j, int &k) {
  k = (int)(n % Z);
  const int t = (int)(n / Z);
  j = t % Y;
  i = t / Y;
}

// One coordinate of a voxel centre.
__device__ __forceinline__ float lift_point(const int idx, const float voxel_size, const float new_origin) {
  return __fadd_rn(__fmul_rn((float)idx, voxel_size), new_origin);
}

// One row of the projection: r . (x, y, z, 1).
__device__ __forceinline__ float lift_row(const float *r, const float x, const float y, const float z) {
  float a = __fmul_rn(r[0], x);
  a = __fmaf_rn(r[1], y, a);
  a = __fmaf_rn(r[2], z, a);
  return __fmaf_rn(r[3], 1.0f, a);
}

// Where a centre lands in a view.  xf, yf: the two quotients (the bilinear rule samples there); xr, yr: the same rounded, the pixel of the
// nearest rule as floats (integers inside the crop when the view is valid); d: the third homogeneous coordinate.
struct LiftPixel {
  float xf, yf, xr, yr, d;
};

// The projection of the centre (x, y, z) by the rows P [3,4] and the validity rule inside the crop (hc, wc), already clamped to the map.
// -> valid; h: where the centre lands.
__device__ __forceinline__ bool lift_project(const float *P, const float x, const float y, const float z, const int hc, const int wc, LiftPixel &h) {
  const float u = lift_row(P, x, y, z);
  const float v = lift_row(P + 4, x, y, z);
  h.d = lift_row(P + 8, x, y, z);
  h.xf = __fdiv_rn(u, h.d);
  h.xr = rintf(h.xf);
  h.yf = __fdiv_rn(v, h.d);
  h.yr = rintf(h.yf);
  return (h.xr >= 0.f) && (h.yr >= 0.f) && (h.xr < (float)wc) && (h.yr < (float)hc) && (h.d > 0.f);
}

// The gate of a measured depth D around the voxel's depth d: 0, negative, NaN and +inf are no measurement and gate nothing; a measurement
// keeps the view where D - front <= d <= D + behind, one rounded sum and one rounded difference.
__device__ __forceinline__ bool lift_gate(const float D, const float d, const float behind, const float front) {
  if (D > 0.f && D < __builtin_inff()) return d <= __fadd_rn(D, behind) && d >= __fsub_rn(D, front);
  return true;
}

// An effective weight counts if it is positive and finite: NaN, 0, negative values and +inf make the view unseen.
__device__ __forceinline__ bool lift_weight_counts(const float w) { return w > 0.f && w < __builtin_inff(); }
