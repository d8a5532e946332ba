// Scoring candidate poses between two rows of the scene state pools (ivx_volume_match_fwd, include/imvoxel.h): matching scenes, scene.py.
//
//   for a candidate M (destination frame -> source frame), over the destination voxels n that are own (W_d > 0), inside the source grid and
//   whose trilinear sample of the source has W_s > 0 ("paired"), and over all channels c, with a = S_d / W_d and b = S_s / W_s:
//       dot += a_c * b_c,   na += a_c * a_c,   nb += b_c * b_c,   pairs += 1
//
// A read-only reduction: nothing is written but the outputs and the scratch.  Geometry chain, inside test, corner order, corner weights and the
// fma chains of the sample are the merge's (csrc/volume_warp.hip), from the same device functions (lift_geometry.h, warp_geometry.h); the file
// is built with -ffp-contract=off and the arithmetic is spelled with the __f*_rn intrinsics in the header's order.
//
// Tiling: the warp's.  ONE GROUP OF G = C/4 LANES OWNS ONE DESTINATION VOXEL, a wave owns tiles of VW = 256 / G (1 .. 64) visited voxels that are
// consecutive in the visiting order (z fastest), and the work of a wave on a tile has the warp's two parts:
//   geometry  lane l < VW alone loads W_d of voxel l of the tile, runs steps 1 - 3 and the eight corner weights, forms the mask of the corners that
//             are read, loads the (up to) eight wsum words, folds W_s, decides "paired" and forms the two reciprocals 1 / W_d and 1 / W_s.  __ballot
//             and __popcll count own and paired voxels.  A tile with no paired voxel ends here: none of its sums is loaded.
//   sums      item e = lane, lane + 64, .. < VW * G is channel word e % G of voxel e / G: base, mask, the three fractions and the two reciprocals come
//             from lane e / G (seven ds_bpermute), the eight 16-byte corner loads and the S_d load are issued before the first use, the sample
//             folds in corner order, a and b are one product each per channel, and the three sums of four products fold in the lane in fp32,
//             channel order.  Each four-term sum is widened at once and added to the lane's three fp64 accumulators.
// A wave walks `iter` consecutive tiles and a workgroup of four waves 4 * iter of them, so the partials of a grid stay few (at most 1024 workgroups
// per candidate).  After the walk: a fixed xor tree over the 64 lanes in fp64, one slot per wave in LDS, lane 0 of the workgroup adds the four
// slots in wave order and stores (dot, na, nb, pairs) of (sample, candidate, workgroup) into the scratch slab; with the first candidate, also the
// own count of (sample, workgroup).  A second launch of one wave per (sample, candidate) sums the slab: lane l adds the partials of workgroups
// l, l + 64, .. in ascending order, then the same xor tree.  No float atomics, no spinning, no dependence between workgroups of a launch; tile
// walk, trees and orders depend on (X, Y, Z, C, step) alone, so the same two states give the same bits in any row of any pool.
//
// Candidates travel by value like the warp's samples (twelve numbers each), MATCH_MAX_CAND = 32 per launch with blockIdx.y the candidate, one
// sample per launch: B * ceil(K / 32) launches and the one that sums.  The other arrangement -- a loop over the candidates inside the workgroup
// that keeps a_c in registers -- was not tried: tools/scene_match_bench.py measures this one (profiles/scene_match.md).
//
// Aligning scenes (ivx_volume_align_fwd, 0.5.8) is the SAME kernel with ALIGN = true, as the merge is the resample kernel with MERGE = true: the
// Gauss-Newton normal equations of the six degrees of freedom of a pose from one launch.  The match instantiation is the code above, unchanged.
//   geometry  also loads the wsum words of the in-grid corners of weight 0, decides "used" (all eight corners in the grid and of positive weight
//             sum), and forms the derivative dD of W_s along the three axes from the eight words (warp_corner_diff, warp_geometry.h).
//   sums      a used voxel loads all eight corner words (the sample still folds only the corners the match folds, so a, b, dot, na, nb keep the
//             match's bits); six more ds_bpermute bring dD and the voxel centre.  Per channel: the three corner derivatives, the gradient, its
//             rotation into the destination frame, the cross product with d = p - about: the Jacobian row J_c (six numbers) and the residual r_c.
//             Per word: 28 four-term fp32 sums in channel order (e, g[6], H upper triangle [21]), each widened at once and added to the lane's 28
//             further fp64 accumulators -- THE DIRECT ARRANGEMENT of include/imvoxel.h: 31 fp64 accumulators per sums lane.  The other one (fold
//             sum_c u u^T, sum_c u r and e over a group's lanes per voxel, apply (I | -[d]x) once per voxel) needs a segmented reduction over
//             groups of G lanes, G not a power of two in general, and was not built: the direct one compiles to 221 VGPRs, two waves
//             per SIMD and no scratch (the resource table is in tools/scene_align_bench.py).
// The tile walk, trees and orders are the match's with 31 sums in place of 3; a partial is 33 words of 8 bytes (31 sums, pairs, used).
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "ivx_common.h"
#include "lift_geometry.h"
#include "warp_geometry.h"

namespace {

constexpr int MATCH_WG = 256, MATCH_WAVES = MATCH_WG / 64;
constexpr int MATCH_MAX_CAND = 32;          // candidates per launch: 12 words each in the kernel arguments
constexpr int MATCH_MAX_WGS = 1024;         // workgroups (partials) per candidate
constexpr int MASK_PAIRED = 1 << 8;         // beside the eight corner bits of a voxel's mask

struct MatchPartial {                       // one workgroup's share of one (sample, candidate): 32 bytes of the scratch slab
  double dot, na, nb;
  long long pairs;
};

struct MatchArgs {
  const float *sum_src, *wsum_src, *sum_dst, *wsum_dst;
  MatchPartial *part;                       // [B, K, wgs]
  long long *own_part;                      // [B, wgs]
  float vs[3], origin[3], origin_src[3];
  int32_t row_src, row_dst;
  int32_t X, Y, Z, G, VW, iter, wgs;        // G = C / 4 lanes per voxel; VW voxels per tile; tiles per wave; workgroups per candidate
  int32_t px, py, pz, Ys, Zs;               // the lattice step and the visited extents ceil(Y / py), ceil(Z / pz)
  int32_t b, k0, K;                         // this launch: sample b, candidates k0 .. k0 + gridDim.y - 1 of K
  long long nvox, nvis;                     // voxels of a row; visited voxels
  float m[MATCH_MAX_CAND][12];              // blockIdx.y is the candidate
};
static_assert(sizeof(MatchArgs) <= 4096, "the candidates travel by value: the argument block must stay under the 4 KB kernel-argument limit");

constexpr int ALIGN_STATS = 31, ALIGN_TERMS = 28;   // (dot, na, nb, e, g[6], H upper triangle [21]); the 28 that the align adds
constexpr int MASK_USED = 1 << 9;           // (align) beside MASK_PAIRED: all eight corners in the grid and of positive weight sum

struct AlignPartial {                       // (align) one workgroup's share of one (sample, candidate): 264 bytes
  double s[ALIGN_STATS];
  long long pairs, used;
};

struct AlignArgs : MatchArgs {              // the match's arguments (part is not used) and the align's own
  AlignPartial *apart;                      // [B, K, wgs]
  float about[3];                           // the point the rotation increments go through
};
static_assert(sizeof(AlignArgs) <= 4096, "the candidates travel by value: the argument block must stay under the 4 KB kernel-argument limit");

template <bool ALIGN>
struct ReduceArgsT {
  const std::conditional_t<ALIGN, AlignPartial, MatchPartial> *part;
  const long long *own_part;
  double *stats_out;                        // [B, K, 3]; (align) [B, K, 31]
  long long *pairs_out, *own_out;           // [B, K]; [B]
  long long *used_out;                      // (align) [B, K]
  int32_t K, wgs;
};

__device__ __forceinline__ float lane4(const float4 &v, const int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// a0 b0 + a1 b1, + a2 b2, + a3 b3: four rounded products, three rounded sums in channel order, widened.
__device__ __forceinline__ double sum4(const float *x, const float *y) {
  return (double)__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(x[0], y[0]), __fmul_rn(x[1], y[1])), __fmul_rn(x[2], y[2])), __fmul_rn(x[3], y[3]));
}

__device__ __forceinline__ double wave_sum(double v) {                  // a fixed xor tree over the 64 lanes
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <bool ALIGN>
__global__ void __launch_bounds__(MATCH_WG) volume_match_kernel(const std::conditional_t<ALIGN, AlignArgs, MatchArgs> a) {
  __shared__ double slot[MATCH_WAVES][ALIGN ? ALIGN_STATS : 3];
  __shared__ int slot_pairs[MATCH_WAVES], slot_own[MATCH_WAVES], slot_used[ALIGN ? MATCH_WAVES : 1];
  const float *m = a.m[blockIdx.y];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // dx, dy, dz with dz fastest; flat offsets in uint32 (wrapping) arithmetic as in csrc/volume_warp.hip: only corners inside the grid are addressed
  const uint32_t uZ = (uint32_t)a.Z, uYZ = (uint32_t)a.Y * (uint32_t)a.Z;
  const uint32_t corner_off[8] = {0u, 1u, uZ, uZ + 1u, uYZ, uYZ + 1u, uYZ + uZ, uYZ + uZ + 1u};
  const float *ws = a.wsum_src + (long long)a.row_src * a.nvox, *wdp = a.wsum_dst + (long long)a.row_dst * a.nvox;
  const float4 *src = (const float4 *)a.sum_src + (long long)a.row_src * a.nvox * a.G;
  const float4 *dst = (const float4 *)a.sum_dst + (long long)a.row_dst * a.nvox * a.G;
  const int items = a.VW * a.G;
  double dot = 0.0, na = 0.0, nb = 0.0;
  double acc[ALIGN ? ALIGN_TERMS : 1] = {};                              // (align) e, g[6], H[21]
  int pairs = 0, own = 0, used = 0;                                      // (per wave, uniform: below 2^31 per workgroup, nvis < 2^31)

  const long long tile0 = ((long long)blockIdx.x * MATCH_WAVES + wv) * a.iter;
  for (int it = 0; it < a.iter; ++it) {
    const long long v0 = (tile0 + it) * a.VW;                            // the first visited voxel of this tile
    if (v0 >= a.nvis) break;                                             // (uniform per wave)
    // ---- geometry: lane l < VW owns visited voxel v0 + l
    uint32_t base = 0, nflat = 0;
    int mask = 0;
    float fx = 0.f, fy = 0.f, fz = 0.f, rd = 0.f, rs = 0.f;
    float dDx = 0.f, dDy = 0.f, dDz = 0.f, cx_ = 0.f, cy_ = 0.f, cz_ = 0.f;   // (align) the derivative of W_s; the voxel centre
    bool is_own = false;
    const long long v = v0 + lane;
    if (lane < a.VW && v < a.nvis) {
      int i, j, k, ix = 0, iy = 0, iz = 0;
      lift_voxel((int)v, a.Ys, a.Zs, i, j, k);                           // v < nvis <= X*Y*Z < 2^31: the visited voxel on the sub-lattice ...
      i *= a.px, j *= a.py, k *= a.pz;                                   // ... and in the grid
      nflat = ((uint32_t)i * (uint32_t)a.Y + (uint32_t)j) * uZ + (uint32_t)k;
      const float wd = wdp[nflat];
      is_own = wd > 0.f;                                                 // (a NaN W_d is not)
      if (is_own) {
        const float px = lift_point(i, a.vs[0], a.origin[0]), py = lift_point(j, a.vs[1], a.origin[1]), pz = lift_point(k, a.vs[2], a.origin[2]);
        const float qx = lift_row(m, px, py, pz), qy = lift_row(m + 4, px, py, pz), qz = lift_row(m + 8, px, py, pz);
        bool in = warp_axis(qx, a.origin_src[0], a.vs[0], a.X, ix, fx);
        in = warp_axis(qy, a.origin_src[1], a.vs[1], a.Y, iy, fy) && in;
        in = warp_axis(qz, a.origin_src[2], a.vs[2], a.Z, iz, fz) && in;
        if (in) {
          base = ((uint32_t)ix * (uint32_t)a.Y + (uint32_t)iy) * uZ + (uint32_t)iz;
          float w[8], wval[8], W = 0.f;
          int ing = 0;                                                   // (align) the corners inside the grid, whatever their weight
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const int cx = ix + (c >> 2), cy = iy + ((c >> 1) & 1), cz = iz + (c & 1);
            w[c] = warp_weight(c, fx, fy, fz);
            const bool inside = cx >= 0 && cx < a.X && cy >= 0 && cy < a.Y && cz >= 0 && cz < a.Z;
            if (inside && w[c] != 0.f) mask |= 1 << c;
            if (ALIGN && inside) ing |= 1 << c;
          }
#pragma unroll
          for (int c = 0; c < 8; ++c) wval[c] = (ALIGN ? ing : mask) >> c & 1 ? ws[(uint32_t)(base + corner_off[c])] : 0.f;      // every load before the first use
#pragma unroll
          for (int c = 0; c < 8; ++c)
            if (mask >> c & 1) W = __fmaf_rn(w[c], wval[c], W);
          if (W > 0.f) {                                                 // paired: own, inside and the state's "seen" rule on the sample
            mask |= MASK_PAIRED;
            rd = __fdiv_rn(1.0f, wd);
            rs = __fdiv_rn(1.0f, W);
            if constexpr (ALIGN) {
              bool all = ing == 0xff;
#pragma unroll
              for (int c = 0; c < 8; ++c) all = all && wval[c] > 0.f;    // (a NaN is not)
              if (all) {
                mask |= MASK_USED;
                dDx = warp_corner_diff(0, wval, fx, fy, fz), dDy = warp_corner_diff(1, wval, fx, fy, fz), dDz = warp_corner_diff(2, wval, fx, fy, fz);
                cx_ = px, cy_ = py, cz_ = pz;
              }
            }
          } else {
            mask = 0;
          }
        }
      }
    }
    own += __popcll(__ballot(is_own));
    const unsigned long long paired = __ballot(mask != 0);
    if (paired == 0ull) continue;                                        // no voxel of the tile is paired for this candidate: no sums are loaded
    pairs += __popcll(paired);
    if constexpr (ALIGN) used += __popcll(__ballot((mask & MASK_USED) != 0));

    // ---- sums: item e is channel word e % G of visited voxel v0 + e / G
    for (int e = lane; e < ((items + 63) & ~63); e += 64) {              // whole waves reach the cross-lane reads
      const int vl = e < items ? e / a.G : 0, c4 = e - vl * a.G;
      const uint32_t vbase = (uint32_t)__shfl((int)base, vl), vn = (uint32_t)__shfl((int)nflat, vl);
      const int vmask = __shfl(mask, vl);
      const float vfx = __shfl(fx, vl), vfy = __shfl(fy, vl), vfz = __shfl(fz, vl), vrd = __shfl(rd, vl), vrs = __shfl(rs, vl);
      float vdD[3] = {0.f, 0.f, 0.f}, vd[3] = {0.f, 0.f, 0.f};
      if constexpr (ALIGN) {
        vdD[0] = __shfl(dDx, vl), vdD[1] = __shfl(dDy, vl), vdD[2] = __shfl(dDz, vl);
        vd[0] = __shfl(cx_, vl), vd[1] = __shfl(cy_, vl), vd[2] = __shfl(cz_, vl);
      }
      if (e >= items || !(vmask & MASK_PAIRED)) continue;                // an unpaired voxel: its sums are not read
      const bool vused = ALIGN && (vmask & MASK_USED);                   // a used voxel reads all eight corners (all in the grid, all W > 0)
      float4 val[8];
#pragma unroll
      for (int c = 0; c < 8; ++c)                                        // every load before the first use
        val[c] = (vmask >> c & 1) || vused ? src[(long long)(uint32_t)(vbase + corner_off[c]) * a.G + c4] : float4{0.f, 0.f, 0.f, 0.f};
      const float4 sd = dst[(long long)vn * a.G + c4];                   // S_d, issued with the corner loads
      float4 smp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (vmask >> c & 1) {
          const float w = warp_weight(c, vfx, vfy, vfz);
          smp.x = __fmaf_rn(w, val[c].x, smp.x);
          smp.y = __fmaf_rn(w, val[c].y, smp.y);
          smp.z = __fmaf_rn(w, val[c].z, smp.z);
          smp.w = __fmaf_rn(w, val[c].w, smp.w);
        }
      const float a0 = __fmul_rn(sd.x, vrd), a1 = __fmul_rn(sd.y, vrd), a2 = __fmul_rn(sd.z, vrd), a3 = __fmul_rn(sd.w, vrd);
      const float b0 = __fmul_rn(smp.x, vrs), b1 = __fmul_rn(smp.y, vrs), b2 = __fmul_rn(smp.z, vrs), b3 = __fmul_rn(smp.w, vrs);
      // four rounded products, three rounded sums in channel order, per statistic; then fp64
      dot += (double)__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a0, b0), __fmul_rn(a1, b1)), __fmul_rn(a2, b2)), __fmul_rn(a3, b3));
      na += (double)__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a0, a0), __fmul_rn(a1, a1)), __fmul_rn(a2, a2)), __fmul_rn(a3, a3));
      nb += (double)__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(b0, b0), __fmul_rn(b1, b1)), __fmul_rn(b2, b2)), __fmul_rn(b3, b3));
      if constexpr (ALIGN) {
        if (vused) {                                                     // selected, never multiplied by zero
          const float av[4] = {a0, a1, a2, a3}, bv[4] = {b0, b1, b2, b3};
          float r[4], J[6][4];                                           // J[i][ch]: component i of the Jacobian row of channel ch of the word
#pragma unroll
          for (int d = 0; d < 3; ++d) vd[d] = __fsub_rn(vd[d], a.about[d]);          // d = p - about
#pragma unroll
          for (int ch = 0; ch < 4; ++ch) {
            float v8[8], g[3];
#pragma unroll
            for (int c = 0; c < 8; ++c) v8[c] = lane4(val[c], ch);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {                             // ((dN - b dD) r_s) / voxel_size
              const float dN = warp_corner_diff(ax, v8, vfx, vfy, vfz);
              g[ax] = __fdiv_rn(__fmul_rn(__fsub_rn(dN, __fmul_rn(bv[ch], vdD[ax])), vrs), a.vs[ax]);
            }
#pragma unroll
            for (int j = 0; j < 3; ++j)                                  // u = R^T grad: R[0][j] g_0, then fma with R[1][j], R[2][j]
              J[j][ch] = __fmaf_rn(m[8 + j], g[2], __fmaf_rn(m[4 + j], g[1], __fmul_rn(m[j], g[0])));
            J[3][ch] = __fsub_rn(__fmul_rn(vd[1], J[2][ch]), __fmul_rn(vd[2], J[1][ch]));          // d x u
            J[4][ch] = __fsub_rn(__fmul_rn(vd[2], J[0][ch]), __fmul_rn(vd[0], J[2][ch]));
            J[5][ch] = __fsub_rn(__fmul_rn(vd[0], J[1][ch]), __fmul_rn(vd[1], J[0][ch]));
            r[ch] = __fsub_rn(bv[ch], av[ch]);
          }
          acc[0] += sum4(r, r);
          int t = 7;
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            acc[1 + i] += sum4(J[i], r);
#pragma unroll
            for (int j = i; j < 6; ++j) acc[t++] += sum4(J[i], J[j]);
          }
        }
      }
    }
  }

  dot = wave_sum(dot), na = wave_sum(na), nb = wave_sum(nb);
  if constexpr (ALIGN) {
#pragma unroll
    for (int i = 0; i < ALIGN_TERMS; ++i) acc[i] = wave_sum(acc[i]);
  }
  if (lane == 0) {
    slot[wv][0] = dot, slot[wv][1] = na, slot[wv][2] = nb;
    slot_pairs[wv] = pairs, slot_own[wv] = own;
    if constexpr (ALIGN) {
#pragma unroll
      for (int i = 0; i < ALIGN_TERMS; ++i) slot[wv][3 + i] = acc[i];
      slot_used[wv] = used;
    }
  }
  __syncthreads();
  if constexpr (ALIGN) {
    if (threadIdx.x == 0) {
      AlignPartial p = {};
      long long o = 0;
#pragma unroll
      for (int q = 0; q < MATCH_WAVES; ++q) {                            // in wave order
#pragma unroll
        for (int i = 0; i < ALIGN_STATS; ++i) p.s[i] += slot[q][i];
        p.pairs += slot_pairs[q], p.used += slot_used[q];
        o += slot_own[q];
      }
      const int k = a.k0 + (int)blockIdx.y;
      a.apart[((long long)a.b * a.K + k) * a.wgs + blockIdx.x] = p;
      if (k == 0) a.own_part[(long long)a.b * a.wgs + blockIdx.x] = o;
    }
    return;
  }
  if (threadIdx.x == 0) {
    MatchPartial p = {0.0, 0.0, 0.0, 0ll};
    long long o = 0;
#pragma unroll
    for (int q = 0; q < MATCH_WAVES; ++q) {                              // in wave order
      p.dot += slot[q][0], p.na += slot[q][1], p.nb += slot[q][2];
      p.pairs += slot_pairs[q];
      o += slot_own[q];
    }
    const int k = a.k0 + (int)blockIdx.y;
    a.part[((long long)a.b * a.K + k) * a.wgs + blockIdx.x] = p;
    if (k == 0) a.own_part[(long long)a.b * a.wgs + blockIdx.x] = o;
  }
}

// One wave per (candidate, sample): lane l adds the partials of workgroups l, l + 64, .. in ascending order, then the fixed xor tree.
template <bool ALIGN>
__global__ void __launch_bounds__(64) volume_match_sum_kernel(const ReduceArgsT<ALIGN> a) {
  const int lane = threadIdx.x, k = blockIdx.x, b = blockIdx.y;
  const auto *p = a.part + ((long long)b * a.K + k) * a.wgs;
  long long pairs = 0, own = 0, used = 0;
  if constexpr (ALIGN) {
    double s[ALIGN_STATS] = {};
    for (int g = lane; g < a.wgs; g += 64) {
#pragma unroll
      for (int i = 0; i < ALIGN_STATS; ++i) s[i] += p[g].s[i];
      pairs += p[g].pairs, used += p[g].used;
      if (k == 0) own += a.own_part[(long long)b * a.wgs + g];
    }
#pragma unroll
    for (int i = 0; i < ALIGN_STATS; ++i) s[i] = wave_sum(s[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      pairs += __shfl_xor(pairs, o);
      own += __shfl_xor(own, o);
      used += __shfl_xor(used, o);
    }
    if (lane == 0) {
      double *out = a.stats_out + ((long long)b * a.K + k) * ALIGN_STATS;
#pragma unroll
      for (int i = 0; i < ALIGN_STATS; ++i) out[i] = s[i];
      a.pairs_out[(long long)b * a.K + k] = pairs;
      a.used_out[(long long)b * a.K + k] = used;
      if (k == 0) a.own_out[b] = own;
    }
  } else {
    double dot = 0.0, na = 0.0, nb = 0.0;
    for (int g = lane; g < a.wgs; g += 64) {
      dot += p[g].dot, na += p[g].na, nb += p[g].nb;
      pairs += p[g].pairs;
      if (k == 0) own += a.own_part[(long long)b * a.wgs + g];
    }
    dot = wave_sum(dot), na = wave_sum(na), nb = wave_sum(nb);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      pairs += __shfl_xor(pairs, o);
      own += __shfl_xor(own, o);
    }
    if (lane == 0) {
      double *s = a.stats_out + ((long long)b * a.K + k) * 3;
      s[0] = dot, s[1] = na, s[2] = nb;
      a.pairs_out[(long long)b * a.K + k] = pairs;
      if (k == 0) a.own_out[b] = own;
    }
  }
}

bool finite_all(const float *p, const long long n) {
  for (long long i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

int match_vw(int C) { return std::min(64, std::max(1, 256 / (C / 4))); }

// The tile walk of a grid: tiles of VW visited voxels, `iter` tiles per wave so that at most MATCH_MAX_WGS workgroups of four waves cover them.
void match_walk(long long nvis, int VW, int &iter, int &wgs) {
  const long long tiles = (nvis + VW - 1) / VW;
  iter = (int)((tiles + (long long)MATCH_WAVES * MATCH_MAX_WGS - 1) / ((long long)MATCH_WAVES * MATCH_MAX_WGS));
  wgs = (int)((tiles + (long long)MATCH_WAVES * iter - 1) / ((long long)MATCH_WAVES * iter));
}

// The workgroups per candidate that any step can need on this grid: the slab is sized for them.
long long match_wgs_cap(long long nvox, int C) {
  const int VW = match_vw(C);
  const long long tiles = (nvox + VW - 1) / VW;
  return std::min<long long>((tiles + MATCH_WAVES - 1) / MATCH_WAVES, MATCH_MAX_WGS);
}

template <bool ALIGN>
int64_t match_scratch_bytes(int32_t B, int32_t K, int32_t X, int32_t Y, int32_t Z, int32_t C) {
  if (B <= 0 || K <= 0 || X <= 0 || Y <= 0 || Z <= 0 || C <= 0 || C % 4 != 0 || (long long)X * Y * Z >= (1ll << 31)) return IVX_ERR_INVALID_ARG;
  const long long cap = match_wgs_cap((long long)X * Y * Z, C);
  const int64_t partial = ALIGN ? sizeof(AlignPartial) : sizeof(MatchPartial);
  return ivx_align_up((int64_t)B * K * cap * partial + (int64_t)B * cap * (int64_t)sizeof(long long), 256);
}

// The one host path of ivx_volume_match_fwd (ALIGN = false: about and used_out are not looked at) and ivx_volume_align_fwd: every check, then
// B * ceil(K / 32) launches and the one that sums.
template <bool ALIGN>
int match_run(const char *what, int32_t B, int32_t K, const int32_t *row_src, const int32_t *row_dst, const float *xform, const float *about,
              const float *origin_dst, const float *origin_src, const float *voxel_size, const int32_t *step, int32_t R_src, int32_t R_dst, int32_t X,
              int32_t Y, int32_t Z, int32_t C, const float *sum_src, const float *wsum_src, const float *sum_dst, const float *wsum_dst,
              int64_t *pairs_out, int64_t *used_out, int64_t *own_out, double *stats_out, void *scratch, ivx_stream_t stream) {
  const bool ptrs = row_src && row_dst && xform && origin_dst && origin_src && voxel_size && sum_src && wsum_src && sum_dst && wsum_dst && pairs_out && own_out && stats_out;
  if (ALIGN)
    IVX_REQUIRE(ptrs && about && used_out, "%s: null argument (the seven host lists, the four pools and the four outputs are all required; step is optional)", what);
  else
    IVX_REQUIRE(ptrs, "%s: null argument (the six host lists, the four pools and the three outputs are all required; step is optional)", what);
  IVX_REQUIRE(scratch, "%s: null scratch (%s tells its size)", what, ALIGN ? "ivx_volume_align_scratch_bytes" : "ivx_volume_match_scratch_bytes");
  IVX_REQUIRE(((uintptr_t)scratch & 7) == 0, "%s: scratch must be 8-byte aligned", what);
  IVX_REQUIRE(B > 0 && K > 0 && R_src > 0 && R_dst > 0 && X > 0 && Y > 0 && Z > 0 && C > 0,
              "%s: bad dims (B, K, R_src, R_dst, X, Y, Z and C must be positive)", what);
  IVX_REQUIRE(C % 4 == 0, "%s: C %% 4 must be 0 (the sums are read as 16-byte words)", what);
  const long long nvox = (long long)X * Y * Z;
  IVX_REQUIRE(nvox < (1ll << 31), "%s: X*Y*Z must be below 2^31", what);
  IVX_REQUIRE((((uintptr_t)sum_src | (uintptr_t)sum_dst) & 15) == 0, "%s: sum_src and sum_dst must be 16-byte aligned", what);
  for (int b = 0; b < B; ++b) {
    IVX_REQUIRE(row_src[b] >= 0 && row_src[b] < R_src, "%s: row_src[%d] = %d is outside [0, %d)", what, b, row_src[b], R_src);
    IVX_REQUIRE(row_dst[b] >= 0 && row_dst[b] < R_dst, "%s: row_dst[%d] = %d is outside [0, %d)", what, b, row_dst[b], R_dst);
  }
  IVX_REQUIRE(finite_all(xform, 12ll * B * K) && finite_all(origin_dst, 3ll * B) && finite_all(origin_src, 3ll * B) && finite_all(voxel_size, 3),
              "%s: xform, origin_dst, origin_src and voxel_size must be finite", what);
  if (ALIGN) IVX_REQUIRE(finite_all(about, 3ll * B), "%s: about must be finite", what);
  IVX_REQUIRE(voxel_size[0] > 0 && voxel_size[1] > 0 && voxel_size[2] > 0, "%s: voxel_size must be positive", what);
  const int32_t one[3] = {1, 1, 1};
  const int32_t *p = step ? step : one;
  IVX_REQUIRE(p[0] >= 1 && p[1] >= 1 && p[2] >= 1, "%s: step must be >= 1 on every axis, got (%d, %d, %d)", what, p[0], p[1], p[2]);

  std::conditional_t<ALIGN, AlignArgs, MatchArgs> a = {};
  a.sum_src = sum_src, a.wsum_src = wsum_src, a.sum_dst = sum_dst, a.wsum_dst = wsum_dst;
  for (int d = 0; d < 3; ++d) a.vs[d] = voxel_size[d];
  a.X = X, a.Y = Y, a.Z = Z, a.G = C / 4, a.VW = match_vw(C), a.nvox = nvox, a.K = K;
  a.px = p[0], a.py = p[1], a.pz = p[2];
  const long long Xs = ((long long)X + p[0] - 1) / p[0];
  a.Ys = (int32_t)(((long long)Y + p[1] - 1) / p[1]), a.Zs = (int32_t)(((long long)Z + p[2] - 1) / p[2]);
  a.nvis = Xs * a.Ys * a.Zs;
  match_walk(a.nvis, a.VW, a.iter, a.wgs);                               // wgs <= match_wgs_cap(nvox, C): the slab holds them
  ReduceArgsT<ALIGN> r = {};
  if constexpr (ALIGN) {
    a.apart = (AlignPartial *)scratch;
    a.own_part = (long long *)(a.apart + (long long)B * K * a.wgs);
    r.part = a.apart, r.used_out = (long long *)used_out;
  } else {
    a.part = (MatchPartial *)scratch;
    a.own_part = (long long *)(a.part + (long long)B * K * a.wgs);
    r.part = a.part;
  }
  for (int b = 0; b < B; ++b) {
    a.b = b, a.row_src = row_src[b], a.row_dst = row_dst[b];
    std::copy(origin_dst + 3 * b, origin_dst + 3 * b + 3, a.origin);
    std::copy(origin_src + 3 * b, origin_src + 3 * b + 3, a.origin_src);
    if constexpr (ALIGN) std::copy(about + 3 * b, about + 3 * b + 3, a.about);
    for (int k0 = 0; k0 < K; k0 += MATCH_MAX_CAND) {
      const int n = std::min(K - k0, MATCH_MAX_CAND);
      a.k0 = k0;
      std::copy(xform + 12ll * ((long long)b * K + k0), xform + 12ll * ((long long)b * K + k0 + n), &a.m[0][0]);
      hipLaunchKernelGGL(volume_match_kernel<ALIGN>, dim3((unsigned)a.wgs, (unsigned)n), dim3(MATCH_WG), 0, (hipStream_t)stream, a);
      IVX_CHECK_LAUNCH(what);
    }
  }
  constexpr int NS = ALIGN ? ALIGN_STATS : 3;
  r.own_part = a.own_part, r.stats_out = stats_out, r.pairs_out = (long long *)pairs_out, r.own_out = (long long *)own_out;
  r.K = K, r.wgs = a.wgs;
  for (int b0 = 0; b0 < B; b0 += 65535) {                                // (grid.y holds 65535 samples)
    const int nb = std::min(B - b0, 65535);
    ReduceArgsT<ALIGN> rb = r;
    rb.part += (long long)b0 * K * a.wgs, rb.own_part += (long long)b0 * a.wgs;
    rb.stats_out += (long long)b0 * K * NS, rb.pairs_out += (long long)b0 * K, rb.own_out += b0;
    if constexpr (ALIGN) rb.used_out += (long long)b0 * K;
    hipLaunchKernelGGL(volume_match_sum_kernel<ALIGN>, dim3((unsigned)K, (unsigned)nb), dim3(64), 0, (hipStream_t)stream, rb);
    IVX_CHECK_LAUNCH(what);
  }
  return IVX_OK;
}

}  // namespace

extern "C" int64_t ivx_volume_match_scratch_bytes(int32_t B, int32_t K, int32_t X, int32_t Y, int32_t Z, int32_t C) {
  return match_scratch_bytes<false>(B, K, X, Y, Z, C);
}

extern "C" int ivx_volume_match_fwd(int32_t B, int32_t K, const int32_t *row_src, const int32_t *row_dst, const float *xform, const float *origin_dst,
                                    const float *origin_src, const float *voxel_size, const int32_t *step, int32_t R_src, int32_t R_dst, int32_t X,
                                    int32_t Y, int32_t Z, int32_t C, const float *sum_src, const float *wsum_src, const float *sum_dst,
                                    const float *wsum_dst, int64_t *pairs_out, int64_t *own_out, double *stats_out, void *scratch, ivx_stream_t stream) {
  return match_run<false>("ivx_volume_match_fwd", B, K, row_src, row_dst, xform, nullptr, origin_dst, origin_src, voxel_size, step, R_src, R_dst, X, Y, Z,
                          C, sum_src, wsum_src, sum_dst, wsum_dst, pairs_out, nullptr, own_out, stats_out, scratch, stream);
}

extern "C" int64_t ivx_volume_align_scratch_bytes(int32_t B, int32_t K, int32_t X, int32_t Y, int32_t Z, int32_t C) {
  return match_scratch_bytes<true>(B, K, X, Y, Z, C);
}

extern "C" int ivx_volume_align_fwd(int32_t B, int32_t K, const int32_t *row_src, const int32_t *row_dst, const float *xform, const float *about,
                                    const float *origin_dst, const float *origin_src, const float *voxel_size, const int32_t *step, int32_t R_src,
                                    int32_t R_dst, int32_t X, int32_t Y, int32_t Z, int32_t C, const float *sum_src, const float *wsum_src,
                                    const float *sum_dst, const float *wsum_dst, int64_t *pairs_out, int64_t *used_out, int64_t *own_out,
                                    double *stats_out, void *scratch, ivx_stream_t stream) {
  return match_run<true>("ivx_volume_align_fwd", B, K, row_src, row_dst, xform, about, origin_dst, origin_src, voxel_size, step, R_src, R_dst, X, Y, Z, C,
                         sum_src, wsum_src, sum_dst, wsum_dst, pairs_out, used_out, own_out, stats_out, scratch, stream);
}
