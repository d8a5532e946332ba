// The trilinear rule of the rigid resample of the scene state, written once as device functions: one axis of step 3 (grid coordinate, inside test,
// floor and fraction) and the weight of a corner from the three fractions (include/imvoxel.h: ivx_volume_warp_fwd steps 3 and 4).
//
// Who uses it.  The resample kernel of csrc/volume_warp.hip in both instantiations (ivx_volume_warp_fwd, ivx_volume_merge_fwd) and the match kernel
// of csrc/volume_match.hip (ivx_volume_match_fwd), whose sample is the merge's: nothing else in csrc/ decides where a source point lies in a grid or
// weighs a corner.  The ALIGN instantiation of the match kernel (ivx_volume_align_fwd) also takes the derivative of the read along an axis from
// here (warp_corner_diff).  The centre of a voxel and the row product come from csrc/lift_geometry.h.
//
// Arithmetic.  Every operation is fp32, round-to-nearest, and spelled with the __f*_rn intrinsics, so nothing is contracted whatever the flags of
// the including file (which is compiled with -ffp-contract=off all the same).
#pragma once
#include <hip/hip_runtime.h>

// One axis of step 3: the grid coordinate g of the source point's coordinate q.  -> inside; i0 = floor(g), f = g - i0 (one rounded difference).
__device__ __forceinline__ bool warp_axis(const float q, const float origin, const float vs, const int N, int &i0, float &f) {
  const float g = __fdiv_rn(__fsub_rn(q, origin), vs);
  if (!(g > -1.0f && g < (float)N)) return false;      // NaN and inf fail as well
  const float fl = floorf(g);
  i0 = (int)fl;
  f = __fsub_rn(g, fl);
  return true;
}

// The weight of corner c = dx * 4 + dy * 2 + dz from the three fractions: (w_x * w_y) * w_z with w_a = 1 - f_a (d = 0) or f_a (d = 1).
__device__ __forceinline__ float warp_weight(const int c, const float fx, const float fy, const float fz) {
  const float wx = c & 4 ? fx : __fsub_rn(1.0f, fx), wy = c & 2 ? fy : __fsub_rn(1.0f, fy), wz = c & 1 ? fz : __fsub_rn(1.0f, fz);
  return __fmul_rn(__fmul_rn(wx, wy), wz);
}

// The derivative of the trilinear read along one axis (0 = x, 1 = y, 2 = z), in cells, from the eight corner values v[c], c = dx * 4 + dy * 2 + dz
// (ivx_volume_align_fwd step 3).  With (p, q) the other two axes in x, y, z order and w_p, w_q their axis weights as in warp_weight:
//   fma(w_p1 * w_q1, v[1,1] - v[0,1], fma(w_p1 * w_q0, .., fma(w_p0 * w_q1, .., fma(w_p0 * w_q0, v[+1 corner] - v[0 corner], +0))))
// -- one rounded product per pair weight, one rounded difference per corner pair, the chain from +0 with q fastest.  All eight values are used.
__device__ __forceinline__ float warp_corner_diff(const int axis, const float *v, const float fx, const float fy, const float fz) {
  const int A = 4 >> axis, P = axis == 0 ? 2 : 4, Q = axis == 2 ? 2 : 1;
  const float fp = axis == 0 ? fy : fx, fq = axis == 2 ? fy : fz;
  const float wp[2] = {__fsub_rn(1.0f, fp), fp}, wq[2] = {__fsub_rn(1.0f, fq), fq};
  float acc = 0.f;
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int c0 = p * P + q * Q;
      acc = __fmaf_rn(__fmul_rn(wp[p], wq[q]), __fsub_rn(v[c0 + A], v[c0]), acc);
    }
  return acc;
}
