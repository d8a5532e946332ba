// Rigid resample of rows of the scene state pools (ivx_volume_warp_fwd, include/imvoxel.h): scenes that turn with their platform, scene.py -- and, as
// a second instantiation of the same kernel, the rigid merge of one row into another (ivx_volume_merge_fwd): scenes that become one.
//
//   dst[i,j,k] = trilinear read of src at  g = (M * centre(i,j,k) - new_origin) / voxel_size,
//
// for the two float fields of a row with the SAME eight corner weights -- volume_sum [R,X,Y,Z,C] fp32 read and written as 16-byte words of four
// channels, wsum [R,X,Y,Z] fp32 -- and the maximum over the read corners for count [R,X,Y,Z] int32.  Out of place: a resample reads the
// neighbours of what it writes.  The operation order is the header's, spelled with the __f*_rn intrinsics and compiled with -ffp-contract=off;
// the centre and the source point are lift_point and lift_row of csrc/lift_geometry.h, so that chain stays written once.
//
// Tiling.  ONE GROUP OF G = C/4 LANES OWNS ONE DESTINATION VOXEL, a wave owns VW = 256 / G voxels (at most 64, at least 1) that are consecutive along z, and
// consecutive voxels go to consecutive lane groups: a wave-wide store of the sums is one contiguous run of 1 KiB (when G divides 64), the wave's
// stores of wsum and count are VW consecutive words.  The work of a wave has two parts:
//   geometry  lane l < VW alone computes steps 1 - 3 of voxel l of the wave (centre, source point, grid coordinate, floor), the eight corner
//             weights, the mask of the corners that are read (inside the grid, weight not 0), then W' and cnt' from the (up to) eight corner words
//             of wsum and count, decides forgetting and stores the two words.  Steps 1 - 3 therefore run once per voxel, not once per lane.
//   sums      item e = lane, lane + 64, .. < VW * G (four steps of the wave for 16 <= C <= 1024) is channel word e % G of voxel e / G: it fetches that voxel's corner base, mask and three
//             fractions from lane e / G (five ds_bpermute), forms the weights by the same three instructions, issues every corner load before
//             the first use and folds them in corner order.  A voxel that is outside, forgotten or sees nothing has mask 0: no load, zeros stored.
// No LDS, no barrier, no atomics: the two parts meet in the wave through cross-lane reads, and no voxel is shared between waves.
// A corner is read by up to eight destination voxels; for a small motion seven of those re-reads are the wave's own or its z / y neighbours'.
// What the counters say (profiles/scene_warp.md, section (d); taken at 16 voxels per wave): the vector L1 absorbs most of them -- the L2 sees 1.2 / 2.5 / 8.6 million requests
// for up to 1.6 / 3.3 / 10.3 million 128-byte corner reads plus the stores -- the L2 hits 42 / 58 / 38 % of what reaches it, and the fabric side fetches
// 2.4 / 1.5 / 3.0 times the row (FETCH_SIZE, doubled as 16-byte-per-lane reads require; Infinity Cache hits included), not the 1.0 of the floor.
//
// VW trades the geometry part, whose instructions a wave pays in full however few of its lanes work in it, against the number of waves and the
// length of a wave's chain of steps.  Tried on an MI355X (profiles/scene_warp.md, section (b); bare C calls, us per row of ScanNet-fast 40x40x16 C256 /
// ScanNet-v1 80x80x32 C64 / the KITTI grid 216x248x12 C64), VW = 1: 25 / 156 / 490; 4: 18 / 44 / 139; 8: 22 / 33 / 108; 16: 24 / 29 / 107; 32: 36 / 34 / 112;
// 64: 63 / 50 / 126 (at C = 256 a row of ScanNet-fast is then 400 waves of 64 steps each).  Both channel counts are fastest where a wave has four steps,
// VW * G = 256, which is the rule (for C < 16 a wave holds its 64 voxels in fewer steps; not measured: no model has so few channels).  64 instead of
// 256 lanes per workgroup at VW = 16: 22 / 30 / 119, not kept.  Re-dealing the workgroup ids so that each of the 8 XCDs, and its L2, walks one
// contiguous eighth of the row instead of every eighth workgroup (at VW = 16): 23 / 29 / 109 against 24 / 29 / 106 in the same run, no gain, not kept.
// Not tried: every lane computing its own geometry.
//
// Merge (the kernel's MERGE flag; the header has the definition).  Geometry chain, corner weights, hand-off and tiling are the warp's, written once.
// The instantiation adds: the SOURCE grid's origin in step 3; on the geometry lane the loads of the destination's own W_d and cnt_d (issued with the
// corner loads), the merged decision W_s > 0, W' = fma(alpha, W_s, W_d), the saturating count, the forget decision and a conditional store; on the
// sums lanes one more 16-byte load, S_d, issued with the corner loads, the one fma with alpha after the fold, and a conditional store.  The mask word
// that travels to the sums lanes carries two bits beside the corners (MASK_STORE, MASK_FORGOT), because "not merged: store nothing" and "forgotten:
// store zeros" are different and a mask of 0 alone cannot say which.  In place: a destination voxel reads only itself in the destination pools, and
// the host refuses a row that is both a source and a destination.  Registers (hipcc -O3 -Rpass-analysis=kernel-resource-usage, gfx950): the warp
// instantiation 58 VGPRs / 48 SGPRs / no scratch / 8 waves per SIMD, as before the template; the merge 62 / 50 / none / 8.
//
// Samples travel by value in the kernel arguments (rows, the twelve numbers of M, the two origins, alpha: 21 words), WARP_MAX_SAMPLES per launch --
// 2784 bytes of arguments in all, under the 4 KB limit, so both instantiations carry 32: nothing is uploaded, and every host list is checked before
// the first launch.
#include <math.h>

#include <algorithm>
#include <vector>

#include "ivx_common.h"
#include "lift_geometry.h"
#include "warp_geometry.h"

#ifndef IVX_WARP_WG
#define IVX_WARP_WG 256
#endif
#ifndef IVX_WARP_VW
#define IVX_WARP_VW 0                       // voxels per wave; 0: 256 / G clamped to 1 .. 64.  1 .. 64 for the A/B builds of tools/scene_warp_bench.py
#endif
static_assert(IVX_WARP_WG % 64 == 0 && IVX_WARP_WG >= 64 && IVX_WARP_WG <= 1024 && IVX_WARP_VW >= 0 && IVX_WARP_VW <= 64, "bad IVX_WARP_WG / IVX_WARP_VW");

namespace {

constexpr int WARP_MAX_SAMPLES = 32;        // samples per launch: 21 words each in the kernel arguments

struct WarpSample {
  int32_t row_src, row_dst;
  float m[12], origin[3];                   // M [3,4] (destination frame -> source frame) and the destination grid's new_origin (the warp's only grid)
  float origin_src[3], alpha;               // the source grid's new_origin (the warp: == origin) and the weight of the source's evidence (MERGE only)
};

struct WarpArgs {
  const float *sum_src, *wsum_src;
  const int32_t *count_src;
  float *sum_dst, *wsum_dst;
  int32_t *count_dst;
  float vs[3], forget_below;
  int32_t X, Y, Z, C, G, VW;                // G = C / 4 lanes per voxel; VW voxels per wave (<= 64)
  long long nvox;
  WarpSample s[WARP_MAX_SAMPLES];           // blockIdx.y is the sample
};
static_assert(sizeof(WarpArgs) <= 4096, "the samples travel by value: the argument block must stay under the 4 KB kernel-argument limit");

// MERGE only, beside the eight corner bits of a voxel's mask: what the sums lanes of a voxel do.  Neither: not merged, nothing is stored.  STORE with
// corner bits: the sample is added to the destination's sums.  STORE | FORGOT (no corner bits): forgotten, zeros are stored and nothing is read.
constexpr int MASK_STORE = 1 << 8, MASK_FORGOT = 1 << 9;

// (One axis of step 3, warp_axis, and the weight of a corner, warp_weight, are csrc/warp_geometry.h: the match kernel shares them.)

// MERGE = false: ivx_volume_warp_fwd, the destination row is written whole.  MERGE = true: ivx_volume_merge_fwd, the sample is added in place to
// the destination voxels that are merged (inside, W_s > 0) and no other voxel is written.
template <bool MERGE>
__global__ void __launch_bounds__(IVX_WARP_WG) volume_warp_kernel(const WarpArgs a) {
  const WarpSample &s = a.s[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (IVX_WARP_WG / 64) + (threadIdx.x >> 6);
  const long long n0 = wave * a.VW;                                      // the first voxel of this wave
  if (n0 >= a.nvox) return;                                              // (uniform per wave)
  const int YZ = a.Y * a.Z;
  // dx, dy, dz with dz fastest.  Flat voxel offsets are formed in uint32 (wrapping) arithmetic: the base of a voxel with an i0 of -1 is negative and
  // Y*Z + Z + 1 may pass 2^31, but the sum for a corner inside the grid is its flat index, below X*Y*Z < 2^31, and only those are addressed.
  const uint32_t uZ = (uint32_t)a.Z, uYZ = (uint32_t)YZ;
  const uint32_t corner_off[8] = {0u, 1u, uZ, uZ + 1u, uYZ, uYZ + 1u, uYZ + uZ, uYZ + uZ + 1u};
  const float *og = MERGE ? s.origin_src : s.origin;                     // the grid that step 3 reads in

  // ---- geometry: lane l < VW owns voxel n0 + l
  uint32_t base = 0;
  int mask = 0;
  float fx = 0.f, fy = 0.f, fz = 0.f;
  const long long n = n0 + lane;
  if (lane < a.VW && n < a.nvox) {
    int i, j, k, ix = 0, iy = 0, iz = 0;
    lift_voxel((int)n, a.Y, a.Z, i, j, k);                                // n < X*Y*Z < 2^31
    const float px = lift_point(i, a.vs[0], s.origin[0]), py = lift_point(j, a.vs[1], s.origin[1]), pz = lift_point(k, a.vs[2], s.origin[2]);
    const float qx = lift_row(s.m, px, py, pz), qy = lift_row(s.m + 4, px, py, pz), qz = lift_row(s.m + 8, px, py, pz);
    bool in = warp_axis(qx, og[0], a.vs[0], a.X, ix, fx);
    in = warp_axis(qy, og[1], a.vs[1], a.Y, iy, fy) && in;
    in = warp_axis(qz, og[2], a.vs[2], a.Z, iz, fz) && in;
    float W = 0.f;
    int cnt = 0;
    bool store = !MERGE;
    if (in) {
      base = ((uint32_t)ix * (uint32_t)a.Y + (uint32_t)iy) * uZ + (uint32_t)iz;
      const float *ws = a.wsum_src + (long long)s.row_src * a.nvox;
      const int32_t *cs = a.count_src + (long long)s.row_src * a.nvox;
      float w[8], wv[8], wd = 0.f;
      int cv[8], cd = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int cx = ix + (c >> 2), cy = iy + ((c >> 1) & 1), cz = iz + (c & 1);
        w[c] = warp_weight(c, fx, fy, fz);
        if (cx >= 0 && cx < a.X && cy >= 0 && cy < a.Y && cz >= 0 && cz < a.Z && w[c] != 0.f) mask |= 1 << c;
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) {                                      // every load before the first use
        const bool rd = mask >> c & 1;
        wv[c] = rd ? ws[(uint32_t)(base + corner_off[c])] : 0.f;
        cv[c] = rd ? cs[(uint32_t)(base + corner_off[c])] : 0;
      }
      if (MERGE) {                                                       // ... the destination's own two words among them
        wd = a.wsum_dst[(long long)s.row_dst * a.nvox + n];
        cd = a.count_dst[(long long)s.row_dst * a.nvox + n];
      }
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (mask >> c & 1) {
          W = __fmaf_rn(w[c], wv[c], W);
          cnt = max(cnt, cv[c]);
        }
      if (MERGE) {
        if (W > 0.f) {                                                   // merged: the state's own "seen" rule on the sample (a NaN W_s is not)
          W = __fmaf_rn(s.alpha, W, wd);
          cnt = (int)min((long long)cd + (long long)cnt, 2147483647ll);
          mask |= MASK_STORE, store = true;
          if (a.forget_below > 0.f && !(W >= a.forget_below)) mask = MASK_STORE | MASK_FORGOT, W = 0.f, cnt = 0;
        } else {
          mask = 0;
        }
      } else if (a.forget_below > 0.f && !(W >= a.forget_below)) {
        mask = 0, W = 0.f, cnt = 0;
      }
    }
    if (store) {
      a.wsum_dst[(long long)s.row_dst * a.nvox + n] = W;
      a.count_dst[(long long)s.row_dst * a.nvox + n] = cnt;
    }
  }

  // ---- sums: item e is channel word e % G of voxel n0 + e / G
  const float4 *src = (const float4 *)a.sum_src + (long long)s.row_src * a.nvox * a.G;
  float4 *dst = (float4 *)a.sum_dst + (long long)s.row_dst * a.nvox * a.G;
  const int items = a.VW * a.G;
  for (int e = lane; e < ((items + 63) & ~63); e += 64) {                // whole waves reach the cross-lane reads
    const int v = e < items ? e / a.G : 0, c4 = e - v * a.G;
    const uint32_t vbase = (uint32_t)__shfl((int)base, v);
    const int vmask = __shfl(mask, v);
    const float vfx = __shfl(fx, v), vfy = __shfl(fy, v), vfz = __shfl(fz, v);
    if (e >= items || n0 + v >= a.nvox) continue;
    if (MERGE && !(vmask & MASK_STORE)) continue;                        // not merged: this voxel's sums are neither read nor written
    float4 val[8], acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 8; ++c)                                          // every load before the first use
      val[c] = vmask >> c & 1 ? src[(long long)(uint32_t)(vbase + corner_off[c]) * a.G + c4] : float4{0.f, 0.f, 0.f, 0.f};
    if (MERGE) acc = vmask & MASK_FORGOT ? float4{0.f, 0.f, 0.f, 0.f} : dst[(n0 + v) * a.G + c4];      // S_d, issued with the corner loads
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
    if (MERGE) {                                                         // (forgotten: no corner bits and no S_d, so fma(alpha, +0, +0) = +0)
      smp.x = __fmaf_rn(s.alpha, smp.x, acc.x);
      smp.y = __fmaf_rn(s.alpha, smp.y, acc.y);
      smp.z = __fmaf_rn(s.alpha, smp.z, acc.z);
      smp.w = __fmaf_rn(s.alpha, smp.w, acc.w);
    }
    dst[(n0 + v) * a.G + c4] = smp;
  }
}

bool finite_all(const float *p, const int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

// Both entries: every check, then the launches.  merge: origin_src and alpha are given and the memory rule is the merge's; else origin_src is
// origin_dst, alpha is NULL and the pools must not overlap.
int resample(const bool merge, const char *what, int32_t B, const int32_t *row_src, const int32_t *row_dst, const float *xform, const float *origin_dst,
             const float *origin_src, const float *alpha, const float *voxel_size, float forget_below, int32_t R_src, int32_t R_dst, int32_t X, int32_t Y,
             int32_t Z, int32_t C, const float *sum_src, const float *wsum_src, const int32_t *count_src, float *sum_dst, float *wsum_dst,
             int32_t *count_dst, ivx_stream_t stream) {
  if (merge)
    IVX_REQUIRE(row_src && row_dst && xform && origin_dst && origin_src && alpha && voxel_size && sum_src && wsum_src && count_src && sum_dst && wsum_dst && count_dst,
                "%s: null argument (the seven host lists and the six pools are all required)", what);
  else
    IVX_REQUIRE(row_src && row_dst && xform && origin_dst && voxel_size && sum_src && wsum_src && count_src && sum_dst && wsum_dst && count_dst,
                "%s: null argument (the five host lists and the six pools are all required)", what);
  IVX_REQUIRE(B > 0 && R_src > 0 && R_dst > 0 && X > 0 && Y > 0 && Z > 0 && C > 0, "%s: bad dims (B, R_src, R_dst, X, Y, Z and C must be positive)", what);
  IVX_REQUIRE(C % 4 == 0, "%s: C %% 4 must be 0 (the sums are read and written as 16-byte words)", what);
  const long long nvox = (long long)X * Y * Z;
  IVX_REQUIRE(nvox < (1ll << 31), "%s: X*Y*Z must be below 2^31", what);
  IVX_REQUIRE((((uintptr_t)sum_src | (uintptr_t)sum_dst) & 15) == 0, "%s: sum_src and sum_dst must be 16-byte aligned", what);
  for (int b = 0; b < B; ++b) {
    IVX_REQUIRE(row_src[b] >= 0 && row_src[b] < R_src, "%s: row_src[%d] = %d is outside [0, %d)", what, b, row_src[b], R_src);
    IVX_REQUIRE(row_dst[b] >= 0 && row_dst[b] < R_dst, "%s: row_dst[%d] = %d is outside [0, %d)", what, b, row_dst[b], R_dst);
  }
  std::vector<int32_t> sorted(row_dst, row_dst + B);
  std::sort(sorted.begin(), sorted.end());
  {
    const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
    IVX_REQUIRE(dup == sorted.end(), "%s: destination rows must be distinct (two samples on row %d)", what, dup == sorted.end() ? 0 : *dup);
  }
  {
    const uintptr_t s0 = (uintptr_t)sum_src, s1 = s0 + (uintptr_t)R_src * nvox * C * 4, d0 = (uintptr_t)sum_dst, d1 = d0 + (uintptr_t)R_dst * nvox * C * 4;
    if (!merge) {
      IVX_REQUIRE(s1 <= d0 || d1 <= s0, "%s: the source and destination sum pools overlap in memory (a resample cannot run in place)", what);
    } else if (!(s1 <= d0 || d1 <= s0)) {
      IVX_REQUIRE(s0 == d0 && R_src == R_dst,
                  "%s: the source and destination sum pools overlap in memory without being the same pool (the same base and R_src == R_dst)", what);
      for (int b = 0; b < B; ++b)
        IVX_REQUIRE(!std::binary_search(sorted.begin(), sorted.end(), row_src[b]),
                    "%s: with one pool as source and destination, row %d is named both as a source and as a destination", what, row_src[b]);
    }
  }
  if (merge) {
    IVX_REQUIRE(finite_all(xform, 12 * B) && finite_all(origin_dst, 3 * B) && finite_all(origin_src, 3 * B) && finite_all(voxel_size, 3),
                "%s: xform, origin_dst, origin_src and voxel_size must be finite", what);
    for (int b = 0; b < B; ++b)
      IVX_REQUIRE(std::isfinite(alpha[b]) && alpha[b] > 0, "%s: alpha[%d] = %g must be finite and > 0", what, b, (double)alpha[b]);
  } else {
    IVX_REQUIRE(finite_all(xform, 12 * B) && finite_all(origin_dst, 3 * B) && finite_all(voxel_size, 3),
                "%s: xform, new_origin and voxel_size must be finite", what);
  }
  IVX_REQUIRE(voxel_size[0] > 0 && voxel_size[1] > 0 && voxel_size[2] > 0, "%s: voxel_size must be positive", what);
  IVX_REQUIRE(std::isfinite(forget_below) && forget_below >= 0, "%s: forget_below must be finite and >= 0", what);

  WarpArgs a = {};
  a.sum_src = sum_src, a.wsum_src = wsum_src, a.count_src = count_src, a.sum_dst = sum_dst, a.wsum_dst = wsum_dst, a.count_dst = count_dst;
  for (int d = 0; d < 3; ++d) a.vs[d] = voxel_size[d];
  a.forget_below = forget_below;
  a.X = X, a.Y = Y, a.Z = Z, a.C = C, a.G = C / 4, a.VW = IVX_WARP_VW ? IVX_WARP_VW : std::min(64, std::max(1, 256 / a.G)), a.nvox = nvox;
  const long long waves = (nvox + a.VW - 1) / a.VW, wgs = (waves + IVX_WARP_WG / 64 - 1) / (IVX_WARP_WG / 64);      // nvox < 2^31: wgs fits a grid
  for (int b0 = 0; b0 < B; b0 += WARP_MAX_SAMPLES) {
    const int n = std::min(B - b0, WARP_MAX_SAMPLES);
    for (int b = 0; b < n; ++b) {
      WarpSample &s = a.s[b];
      s.row_src = row_src[b0 + b], s.row_dst = row_dst[b0 + b];
      std::copy(xform + 12 * (b0 + b), xform + 12 * (b0 + b + 1), s.m);
      std::copy(origin_dst + 3 * (b0 + b), origin_dst + 3 * (b0 + b + 1), s.origin);
      std::copy(origin_src + 3 * (b0 + b), origin_src + 3 * (b0 + b + 1), s.origin_src);
      s.alpha = merge ? alpha[b0 + b] : 1.0f;
    }
    if (merge)
      hipLaunchKernelGGL(volume_warp_kernel<true>, dim3((unsigned)wgs, (unsigned)n), dim3(IVX_WARP_WG), 0, (hipStream_t)stream, a);
    else
      hipLaunchKernelGGL(volume_warp_kernel<false>, dim3((unsigned)wgs, (unsigned)n), dim3(IVX_WARP_WG), 0, (hipStream_t)stream, a);
    IVX_CHECK_LAUNCH(what);
  }
  return IVX_OK;
}

}  // namespace

extern "C" int ivx_volume_warp_fwd(int32_t B, const int32_t *row_src, const int32_t *row_dst, const float *xform, const float *new_origin,
                                   const float *voxel_size, float forget_below, int32_t R_src, int32_t R_dst, int32_t X, int32_t Y, int32_t Z, int32_t C,
                                   const float *sum_src, const float *wsum_src, const int32_t *count_src, float *sum_dst, float *wsum_dst,
                                   int32_t *count_dst, ivx_stream_t stream) {
  return resample(false, "ivx_volume_warp_fwd", B, row_src, row_dst, xform, new_origin, new_origin, nullptr, voxel_size, forget_below, R_src, R_dst, X, Y, Z, C,
                  sum_src, wsum_src, count_src, sum_dst, wsum_dst, count_dst, stream);
}

extern "C" int ivx_volume_merge_fwd(int32_t B, const int32_t *row_src, const int32_t *row_dst, const float *xform, const float *origin_dst,
                                    const float *origin_src, const float *alpha, const float *voxel_size, float forget_below, int32_t R_src, int32_t R_dst,
                                    int32_t X, int32_t Y, int32_t Z, int32_t C, const float *sum_src, const float *wsum_src, const int32_t *count_src,
                                    float *sum_dst, float *wsum_dst, int32_t *count_dst, ivx_stream_t stream) {
  return resample(true, "ivx_volume_merge_fwd", B, row_src, row_dst, xform, origin_dst, origin_src, alpha, voxel_size, forget_below, R_src, R_dst, X, Y, Z, C,
                  sum_src, wsum_src, count_src, sum_dst, wsum_dst, count_dst, stream);
}
