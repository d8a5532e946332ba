// Fused image-to-voxel unprojection (projection + nearest gather + view mean + zero fill + valid
// mask) for a whole batch in one launch.  Replaces mmdet3d/models/detectors/imvoxelnet.py:58-76,
// :132-141 (get_points) and :145-160 (backproject); see include/imvoxel.h.
//
// HBM-bound: the volume [B,X,Y,Z,C] is written exactly once (coalesced: a voxel's C channels are
// contiguous and consecutive voxels are consecutive in memory), the feature maps are read through
// L2 / Infinity Cache (neighbouring voxels hit neighbouring pixels), nothing else is materialised
// (the reference materialises [V,C,N] and makes four more passes over it).
//
// Work split: a group of LPV lanes (power of two, >= ceil(C/VEC) up to 64) owns one voxel; each
// lane owns VEC consecutive channels (float4 when C % 4 == 0).  The per-view projection is spread
// over the group's lanes -- lane g projects view (chunk*LPV + g) -- and the resulting pixel
// offsets are broadcast with wavefront shuffles, so a 50-view scene costs one projection per
// lane per LPV views instead of one per lane per view.
//
// Arithmetic parity (measured against the imported reference, tests/golden/backproject_cases.npz):
//   point, (u,v,d), xf, yf, xr, yr, valid: lift_geometry.h, the one statement of the geometry chain; both kernels below call it
//   mean    = (sum over valid views in view order) / float(count)  (IEEE divide), 0 if count == 0   (bp_divides below)
// This file is compiled with -ffp-contract=off.
//
// Optional bilinear sampling (BP_BILINEAR, ivx_backproject_fwd_ex; an extra mode outside the reference-parity claims, defined in
// include/imvoxel.h and pinned to the fp64 reference of tests/ref_unproject.py).  Validity, mask and count are the nearest rule's; with
// the unrounded quotients xf, yf of lift_project:
//   x0 = floor(xf), x1 = x0 + 1, y0 = floor(yf), y1 = y0 + 1, each clamped to the crop (border rule)
//   ax = xf - floor(xf), ay = yf - floor(yf), bx = 1 - ax, by = 1 - ay                         (__fsub_rn)
//   w00 = bx * by, w10 = ax * by, w01 = bx * ay, w11 = ax * ay                                 (__fmul_rn)
//   sample = fma(w11, f11, fma(w01, f01, fma(w10, f10, w00 * f00)))                            (__fmul_rn, then three __fmaf_rn)
// (bp_bilinear_sample below, the one function every mode and element type calls), then the same view sum and division.
#include "ivx_common.h"
#include "lift_geometry.h"
#include <stdlib.h>
#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The mean of a sum over the evidence it was gathered with, a view count (int) or a weight sum (float): sum / (float)evidence where bp_divides,
// else 0; the mask is bp_seen.  Stated once for the lift's stores and for volume_normalize_kernel.  A count divides when it is != 0 and is seen
// when it is > 0; a weight sum divides and is seen when it is > 0 (NaN: neither).  The guarded division itself stays a conditional expression in
// the two kernels: inside a helper the compiler turns it into a division on every path and a select (profiles/lift_one_geometry.md).
template <typename E>
__device__ __forceinline__ bool bp_divides(const E ev) {
  if constexpr (std::is_floating_point_v<E>) return ev > 0.f;
  else return ev != 0;
}
template <typename E>
__device__ __forceinline__ bool bp_seen(const E ev) { return ev > 0; }

struct BpParams {
  const float *feat;        // [B*V, FH, FW, C]
  const float *proj;        // [B, V, 12]
  const float *new_origin;  // [B, 3]
  const int *crop_hw;       // [B, 2]
  float *volume;            // [B, N, C]
  uint8_t *valid;           // [B, N]  (accumulate mode: written with mean_out, may be NULL)
  int *count;               // [B, N]  (sum / accumulate mode: number of views that saw the voxel)
  void *mean_out;           // accumulate mode: [B, N, C] in the feature type, the mean of the running sum, or NULL
  int first;                // accumulate mode: != 0 starts the running (sum, count) from zero without reading them
  float vs0, vs1, vs2;
  int V, FH, FW, C;
  int X, Y, Z;
  int N;        // X*Y*Z
  int nchunk;   // ceil(C / VEC)
  int lpv_log2; // lanes per voxel = 1 << lpv_log2
  float *pmax;  // single-view lift only: per-workgroup max |volume| goes to pmax[blockIdx.y * gridDim.x + blockIdx.x], or NULL
  int nblk, q;  // multi-view kernel: voxel blocks per sample and per XCD (grid.x = 8 * q, see the kernel's block order); q = 0: plain order (A/B)
};
// GATHER instantiations of backproject_mean_kernel (the others keep BpParams as their one argument): feat is a pool [S, FH, FW, C], proj a pool
// [S, 12], and view v of sample b is slot view_slot[b * V + v] of both
struct BpGatherParams : BpParams {
  const int *view_slot;     // [B, V]
  int S;
};
// ROWS instantiations (ivx_backproject_lists_fwd; scene batches): the gathered form whose sample b reads and writes row row[b] (NULL: b) of the
// R-row state / output pools and, in BP_ACCUM, starts from zero by first_list[b] (NULL: `first` for every sample)
struct BpListParams : BpGatherParams {
  const int *row;           // [B] or NULL
  const int *first_list;    // [B] or NULL
  int R;
};
// WEIGHTED instantiations (ivx_backproject_weighted_fwd; fading scenes): the ROWS form whose views carry weights and whose state has a weight sum
struct BpWeightParams : BpListParams {
  const float *view_weight; // [S] or NULL (= 1)
  const float *decay;       // [B] or NULL (= 1); BP_ACCUM
  float forget_below;       // BP_ACCUM: a faded weight sum below it forgets the voxel; 0 forgets nothing
  float *wsum;              // [R, N]  BP_ACCUM: the running weight sum, beside count
};
// MAPPED instantiations (ivx_backproject_mapped_fwd; pixel maps): the WEIGHTED form whose views bring a per-pixel confidence and / or a depth map
struct BpMapParams : BpWeightParams {
  const float *pixel_weight; // [S, FH, FW] or NULL (= 1)
  const float *depth;        // [S, FH, FW] or NULL (no gate)
  float behind, front;       // the gate around a measured depth D: the view counts where D - front <= d <= D + behind; read only with depth
};

// MODE BP_MEAN: the reference's view mean + valid mask.  BP_SUM (view-sharded multi-GPU mode): the raw sum over
// this rank's views and the per-voxel view count, to be all-reduced and normalised by volume_normalize_kernel.
// BP_ACCUM (streaming scenes): the accumulator and the counter of a voxel start from the stored fp32 sum / count (from zero with
// p.first, the state is then not read), this call's views are added in view order, and the new sum / count are stored back; with
// p.mean_out the same pass also stores the mean (type T) and the valid mask.  The additions are the same __fadd_rn chain in the same
// order as one BP_MEAN launch over all the views, so views that arrive in order give that launch's bits however they are chunked.
// One lane group owns a voxel in every mode: no atomics.  VEC 4 only for BP_SUM / BP_ACCUM.
// T = float (the reference's precision) or __bf16 (optional storage mode: features / volume stored as bf16, the view sum
// and the division in fp32, one rounding at the store; VEC 4 only).
enum { BP_SUM = 0, BP_MEAN = 1, BP_ACCUM = 2 };
// SAMP BP_NEAREST: the reference's gather (the code below is what it was before the parameter existed).  BP_BILINEAR: the projecting
// lane also leaves the clamped steps to the other three corners and the two fractions; the group receives them through __shfl like the
// pixel offset, and every lane blends its channel chunk from four 16-byte loads, one chunk at a time (4 corner vectors live, not 16).
enum { BP_NEAREST = 0, BP_BILINEAR = 1 };
// The bilinear sample of one channel in the ONE fixed order of include/imvoxel.h.  w = {w00, w10, w01, w11}.
__device__ __forceinline__ float bp_bilinear_sample(const float f00, const float f10, const float f01, const float f11, const float *w) {
  float s = __fmul_rn(w[0], f00);
  s = __fmaf_rn(w[1], f10, s);
  s = __fmaf_rn(w[2], f01, s);
  return __fmaf_rn(w[3], f11, s);
}
__device__ __forceinline__ void bp_bilinear_weights(const float ax, const float ay, float *w) {
  const float bx = __fsub_rn(1.0f, ax), by = __fsub_rn(1.0f, ay);
  w[0] = __fmul_rn(bx, by);
  w[1] = __fmul_rn(ax, by);
  w[2] = __fmul_rn(bx, ay);
  w[3] = __fmul_rn(ax, ay);
}
// GATHER (ivx_backproject_gather_fwd; sliding-window scenes): the views are read through a slot list instead of from one contiguous stack.  Only
// the projecting lane's addressing differs -- which map and which projection rows view v is --; the broadcast, the sample function, the view-order
// __fadd_rn chain, the division and the stores are the code of every other mode, so the result is bit for bit the non-gathered launch over a
// contiguous copy of the listed views.  A slot outside [0, S) is tested before any address is formed: that view sees no voxel (off stays -1).
// ROWS (ivx_backproject_lists_fwd; scene batches, ragged one-shot batches; GATHER forms only): sample b keeps its state and writes its outputs in
// row r = row[b] of pools of R rows, and in BP_ACCUM starts from zero by its own flag.  Only WHERE the state / outputs live and WHETHER the state is
// read differ; everything between is the code above, so row r is bit for bit what the B = 1 launch over the sample's listed views leaves there.  A
// row outside [0, R) ends the whole workgroup before any address is formed (r depends on blockIdx.y alone: no lane of it stays behind).  A list of
// nothing but unseen views adds nothing: with `first` the row becomes zero sum / zero count (mean 0, valid 0), without it the state is stored back
// as it was loaded (16-byte loads and stores, no arithmetic: every bit pattern survives).
// WEIGHTED (ivx_backproject_weighted_fwd; fading scenes; ROWS forms only; the definition is in include/imvoxel.h): the projecting lane loads the
// weight of its view next to its projection rows (both addresses come from the slot alone, so the two loads overlap) -- a weight that fails
// w > 0 && w < inf makes the view unseen like a failed validity test: no feature address of it is formed -- and broadcasts it with the pixel offset; the view sum is S = fma(w, sample, S), and the weight sum W lives with cnt (every lane of
// the group carries both, lane g == 0 stores them).  BP_ACCUM fades the state it read, S *= lambda and W *= lambda unless lambda == 1 (uniform
// per sample), and forgets the voxel whose faded W is below p.forget_below (> 0).  The mean divides by W.  With unit weights fma(1, f, S) is the
// __fadd_rn of the other forms and W == (float)cnt, so volume / count / mean / valid are theirs bit for bit.
// MAPPED (ivx_backproject_mapped_fwd; pixel maps; WEIGHTED forms only; the definition is in include/imvoxel.h): once its validity test has passed, the
// projecting lane reads the two maps at the NEAREST pixel of its view (the pixel the validity rule rounds to, under BP_BILINEAR too, where `off` is
// corner 00 and the index is formed apart); both addresses come from slot and pixel alone, so the two loads overlap and no address depends on a
// map's value.  A measured depth D (D > 0 && D < inf) keeps the view only where D - front <= d <= D + behind (one rounded sum, one rounded
// difference); the weight becomes w = wt * pixel_weight (one rounded product) and must pass w > 0 && w < inf again.  A view that fails either test
// is unseen (off stays -1), and `wt` carries the effective weight through the existing __shfl: the group's inner loop is the WEIGHTED one.
template <int VEC, int MODE = BP_MEAN, typename T = float, int SAMP = BP_NEAREST, bool GATHER = false, bool ROWS = false, bool WEIGHTED = false,
          bool MAPPED = false>
__global__ __launch_bounds__(256) void backproject_mean_kernel(
    const std::conditional_t<MAPPED, BpMapParams, std::conditional_t<WEIGHTED, BpWeightParams, std::conditional_t<ROWS, BpListParams, std::conditional_t<GATHER, BpGatherParams, BpParams>>>> p) {
  static_assert(!ROWS || (GATHER && VEC == 4 && MODE != BP_SUM), "the ROWS forms are the gathered mean / accumulate kernels");
  static_assert(!WEIGHTED || ROWS, "the WEIGHTED forms are ROWS forms");
  static_assert(!MAPPED || WEIGHTED, "the MAPPED forms are WEIGHTED forms");
  static_assert(VEC == 4 || MODE == BP_MEAN, "VEC 1 is the fp32 mean of a view stack");
  typedef T tv4 __attribute__((ext_vector_type(4)));
  const int b = blockIdx.y;
  int r = b;                               // the row of the state / outputs of this sample
  int first = p.first;
  if constexpr (ROWS) {
    if (p.row) r = p.row[b];
    if (r < 0 || r >= p.R) return;
    if (p.first_list) first = p.first_list[b];
  }
  float lam = 1.0f;                        // WEIGHTED BP_ACCUM: the decay of this sample, loaded with the row and the flag (b < B: no guard needed)
  if constexpr (WEIGHTED && MODE == BP_ACCUM) {
    if (p.decay) lam = p.decay[b];
  }
  const int lpv = 1 << p.lpv_log2;
  const int lane = threadIdx.x & 63;
  const int g = lane & (lpv - 1);        // lane inside the voxel group
  const int gbase = lane & ~(lpv - 1);   // first lane of the group inside the wave
  const int vox_per_block = 256 >> p.lpv_log2;
  // Optional XCD-contiguous block order (IVX_BP_ORDER=1; round 5, the round-4 verdict's item 5): workgroup w runs on XCD w % 8 (observed
  // dispatch rule) and grid.x = 8 * q, so XCD x gets the x-th contiguous eighth of a sample's voxel blocks -- an x-slab of the volume.
  // MEASURED AND NOT ADOPTED (profiles/r05_unprojection_block_order.md): ScanNet, 50 views, 80x80x32: 0.300 -> 0.370 ms per 2 scenes,
  // FETCH_SIZE 871 -> 928 MB per scene, L2 hits -29 %.  An x-slab is seen by all 50 views (a band of ~1 MB of each 4.9 MB map: 50 MB per
  // XCD against 4 MB of L2), neighbouring voxels land 4-5 feature pixels apart, and the reuse that exists -- voxels along one camera ray --
  // is far apart in any voxel order; dealt round-robin the eight XCDs at least walk the same region at the same time, so the Infinity
  // Cache serves their common lines once.  The values do not depend on the order (bit-exact tests run both).
  const int vb = p.q ? (int)(blockIdx.x & 7) * p.q + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  if (vb >= p.nblk) return;              // padding of the last XCD's range (whole workgroups; no barrier in this kernel)
  const int n = vb * vox_per_block + (threadIdx.x >> p.lpv_log2);
  const bool active = n < p.N;
  const int nn = active ? n : p.N - 1;

  int i, j, k;
  lift_voxel(nn, p.Y, p.Z, i, j, k);
  const float *no = p.new_origin + b * 3;
  const float px = lift_point(i, p.vs0, no[0]), py = lift_point(j, p.vs1, no[1]), pz = lift_point(k, p.vs2, no[2]);
  const int hc = min(p.crop_hw[b * 2 + 0], p.FH), wc = min(p.crop_hw[b * 2 + 1], p.FW);   // slice semantics (detectors/imvoxelnet.py:69): clamped to the map

  constexpr int MAXCH = 4;  // channel chunks per lane when ceil(C/VEC) > 64 lanes (C up to 1024 for VEC 4)
  float acc[MAXCH][VEC];
#pragma unroll
  for (int q = 0; q < MAXCH; ++q)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[q][e] = 0.f;
  int cnt = 0;
  float wacc = 0.f;           // WEIGHTED: the weight sum W of this voxel
  if constexpr (MODE == BP_ACCUM) {
    if (active && !first) {              // the running state of this voxel (16-byte loads, coalesced as the stores below)
      const float *run = p.volume + ((size_t)r * p.N + n) * p.C;
#pragma unroll
      for (int q = 0; q < MAXCH; ++q) {
        const int ch = g + q * lpv;
        if (ch < p.nchunk) {
          const f32x4 x = *reinterpret_cast<const f32x4 *>(run + ch * 4);
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[q][e] = x[e];
        }
      }
      cnt = p.count[(size_t)r * p.N + n];
      if constexpr (WEIGHTED) {          // fade, then forget: only a state that was read
        wacc = p.wsum[(size_t)r * p.N + n];
        if (lam != 1.0f) {
#pragma unroll
          for (int q = 0; q < MAXCH; ++q)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[q][e] = __fmul_rn(lam, acc[q][e]);
          wacc = __fmul_rn(lam, wacc);
        }
        if (p.forget_below > 0.f && !(wacc >= p.forget_below)) {
#pragma unroll
          for (int q = 0; q < MAXCH; ++q)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[q][e] = 0.f;
          wacc = 0.f;
          cnt = 0;
        }
      }
    }
  }

  for (int v0 = 0; v0 < p.V; v0 += lpv) {
    // lane g projects view v0 + g
    const int v = v0 + g;
    int off = -1;
    int step = 0;               // BP_BILINEAR: bit 0 = x1 is one pixel right of x0, bit 1 = y1 is one row below y0 (0 where the clamp joins them)
    float ax = 0.f, ay = 0.f;   // BP_BILINEAR: the fractions
    int slot = 0;               // GATHER: the slot of this view
    float wt = 1.0f;            // WEIGHTED: its weight
    bool listed = v < p.V;
    if constexpr (GATHER) {
      if (listed) {
        slot = p.view_slot[b * p.V + v];
        listed = slot >= 0 && slot < p.S;
      }
    }
    if constexpr (WEIGHTED) {      // loaded beside the projection rows (both need the slot only); tested with the validity below
      if (listed && p.view_weight) wt = p.view_weight[slot];
    }
    if (listed) {
      LiftPixel h;
      bool ok = lift_project(p.proj + (GATHER ? (size_t)slot : (size_t)b * p.V + v) * 12, px, py, pz, hc, wc, h);
      if constexpr (WEIGHTED) ok = ok && lift_weight_counts(wt);     // NaN, 0, negative and inf: an unseen view (off stays -1)
      if constexpr (MAPPED) {
        if (ok) {                 // the nearest pixel is inside the crop, hence inside the map: slot in [0, S), (int)yr in [0, FH), (int)xr in [0, FW)
          const int pix = (slot * p.FH + (int)h.yr) * p.FW + (int)h.xr;
          const float D = p.depth ? p.depth[pix] : 0.f;
          const float pw = p.pixel_weight ? p.pixel_weight[pix] : 1.0f;
          ok = lift_gate(D, h.d, p.behind, p.front);
          if (p.pixel_weight) {
            wt = __fmul_rn(wt, pw);
            ok = ok && lift_weight_counts(wt);
          }
        }
      }
      if (ok) off = (((GATHER ? slot : b * p.V + v) * p.FH + (int)h.yr) * p.FW + (int)h.xr);
      if constexpr (SAMP == BP_BILINEAR) {
        if (ok) {               // a valid sample: xf in [-0.5, wc - 0.5], so the floors are in [-1, wc - 1] and fit an int
          const float fx = floorf(h.xf), fy = floorf(h.yf);
          ax = __fsub_rn(h.xf, fx);
          ay = __fsub_rn(h.yf, fy);
          const int x0 = max((int)fx, 0), x1 = min((int)fx + 1, wc - 1);     // x0 <= wc - 1 and x1 >= 0 already
          const int y0 = max((int)fy, 0), y1 = min((int)fy + 1, hc - 1);
          step = (x1 - x0) | ((y1 - y0) << 1);
          off = (((GATHER ? slot : b * p.V + v) * p.FH + y0) * p.FW + x0);   // corner 00
        }
      }
    }
    const int nv = (p.V - v0) < lpv ? (p.V - v0) : lpv;
    for (int s = 0; s < nv; ++s) {
      const int o = __shfl(off, gbase + s, 64);
      int dx = 0, dy = 0;       // BP_BILINEAR: element offsets from corner 00 to corners 10 and 01
      float w[4];
      float ws = 1.0f;          // WEIGHTED: the weight of view v0 + s
      if constexpr (WEIGHTED) ws = __shfl(wt, gbase + s, 64);
      if constexpr (SAMP == BP_BILINEAR) {
        const int st = __shfl(step, gbase + s, 64);
        const float axs = __shfl(ax, gbase + s, 64), ays = __shfl(ay, gbase + s, 64);
        dx = (st & 1) * p.C;
        dy = (st >> 1) * p.FW * p.C;
        bp_bilinear_weights(axs, ays, w);
      }
      if (o >= 0) {
        ++cnt;
        if constexpr (WEIGHTED) wacc = __fadd_rn(wacc, ws);
        const T *src = reinterpret_cast<const T *>(p.feat) + (size_t)o * p.C;
#pragma unroll
        for (int q = 0; q < MAXCH; ++q) {
          const int ch = g + q * lpv;
          if (ch < p.nchunk) {
            if constexpr (SAMP == BP_BILINEAR && VEC == 4) {
              const tv4 c00 = *reinterpret_cast<const tv4 *>(src + ch * 4);
              const tv4 c10 = *reinterpret_cast<const tv4 *>(src + dx + ch * 4);
              const tv4 c01 = *reinterpret_cast<const tv4 *>(src + dy + ch * 4);
              const tv4 c11 = *reinterpret_cast<const tv4 *>(src + dy + dx + ch * 4);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float f = bp_bilinear_sample((float)c00[e], (float)c10[e], (float)c01[e], (float)c11[e], w);
                if constexpr (WEIGHTED) acc[q][e] = __fmaf_rn(ws, f, acc[q][e]);
                else acc[q][e] = __fadd_rn(acc[q][e], f);
              }
            } else if constexpr (SAMP == BP_BILINEAR) {
              acc[q][0] = __fadd_rn(acc[q][0], bp_bilinear_sample((float)src[ch], (float)src[dx + ch], (float)src[dy + ch], (float)src[dy + dx + ch], w));
            } else if constexpr (VEC == 4) {
              const tv4 xr = *reinterpret_cast<const tv4 *>(src + ch * 4);
              const f32x4 x = {(float)xr[0], (float)xr[1], (float)xr[2], (float)xr[3]};
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                if constexpr (WEIGHTED) acc[q][e] = __fmaf_rn(ws, x[e], acc[q][e]);
                else acc[q][e] = __fadd_rn(acc[q][e], x[e]);
              }
            } else {
              acc[q][0] = __fadd_rn(acc[q][0], (float)src[ch]);
            }
          }
        }
      }
    }
  }

  if (!active) return;
  // The stores of every form.  The evidence of the voxel is its weight sum (WEIGHTED) or its view count; `run` is the fp32 state of BP_ACCUM
  // (stored as it stands: a list of unseen views puts the loaded bits back, no arithmetic), `out` the volume in the feature type: the mean of
  // BP_MEAN and of BP_ACCUM with mean_out, the raw sum of BP_SUM.
  std::conditional_t<WEIGHTED, float, int> ev;
  if constexpr (WEIGHTED) ev = wacc;
  else ev = cnt;
  const float den = (float)ev;
  const size_t at = (size_t)r * p.N + n;
  float *run = p.volume + at * p.C;
  T *out = MODE != BP_ACCUM ? reinterpret_cast<T *>(p.volume) + at * p.C : p.mean_out ? reinterpret_cast<T *>(p.mean_out) + at * p.C : nullptr;
  const bool has_out = MODE != BP_ACCUM || out;     // BP_ACCUM without mean_out updates the state alone
#pragma unroll
  for (int q = 0; q < MAXCH; ++q) {
    const int ch = g + q * lpv;
    if (ch < p.nchunk) {
      f32x4 s;
      tv4 y;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        s[e] = acc[q][e];
        y[e] = (T)(MODE == BP_SUM ? acc[q][e] : bp_divides(ev) ? __fdiv_rn(acc[q][e], den) : 0.f);
      }
      if constexpr (MODE == BP_ACCUM) *reinterpret_cast<f32x4 *>(run + ch * 4) = s;
      if constexpr (VEC == 1) out[ch] = y[0];
      else if (has_out) *reinterpret_cast<tv4 *>(out + ch * 4) = y;
    }
  }
  if (g == 0) {
    if constexpr (MODE != BP_MEAN) p.count[at] = cnt;
    if constexpr (WEIGHTED && MODE == BP_ACCUM) p.wsum[at] = wacc;
    if (MODE != BP_SUM && has_out) p.valid[at] = bp_seen(ev) ? 1 : 0;
  }
}

// The mean of a stored state, by the lift's own division and mask: out[n,:] = bp_divides(evidence[n]) ? sum[n,:] / evidence[n] : 0, valid =
// bp_seen(evidence[n]).  E = int: a (sum, count) state (detectors/imvoxelnet.py:70-74 after the all-reduce of the per-rank partial sums, or the
// running sums of a streaming scene); E = float: a (sum, weight sum) state (ivx_volume_wmean_fwd).  out == sum: in place (ivx_volume_normalize_fwd); otherwise the sums stay intact
// and T may be __bf16 (one rounding at the store).  One float4 of sums per thread.
template <typename T, typename E>
__global__ __launch_bounds__(256) void volume_normalize_kernel(const float *sum, T *out, const E *evidence, uint8_t *valid, long long total4, int C4) {
  typedef T tv4 __attribute__((ext_vector_type(4)));
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
    const long long vox = i / C4;
    const E ev = evidence[vox];
    const f32x4 x = *reinterpret_cast<const f32x4 *>(sum + i * 4);
    const float den = (float)ev;
    tv4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = (T)(bp_divides(ev) ? __fdiv_rn(x[e], den) : 0.f);
    *reinterpret_cast<tv4 *>(out + i * 4) = y;
    if (i % C4 == 0) valid[vox] = bp_seen(ev) ? 1 : 0;
  }
}

// Single-view specialisation (KITTI, SUN RGB-D: V == 1).  With one view the mean is the gathered value itself, so no
// accumulation is needed and the roles flip: a group of LPV lanes owns LPV consecutive voxels, lane g projects voxel
// n0 + g (one projection per lane instead of one per group), then the group walks its voxels and every lane
// copies its VEC channels of voxel n0 + s from the pixel that voxel hit (offset broadcast with __shfl).  Per
// 1 KiB of volume written a wave issues a handful of instructions, so the kernel is bound by the volume write.
template <int VEC>
__global__ __launch_bounds__(256) void backproject_single_view_kernel(const BpParams p) {
  const int b = blockIdx.y;
  const int lpv = 1 << p.lpv_log2;
  const int lane = threadIdx.x & 63;
  const int g = lane & (lpv - 1);
  const int gbase = lane & ~(lpv - 1);
  const int group = (blockIdx.x * 256 + threadIdx.x) >> p.lpv_log2;   // global group index
  const long long n0 = (long long)group * lpv;
  const long long n = n0 + g;
  int off = -1;
  if (n < p.N) {
    int i, j, k;
    lift_voxel(n, p.Y, p.Z, i, j, k);
    const float *no = p.new_origin + b * 3;
    const float px = lift_point(i, p.vs0, no[0]), py = lift_point(j, p.vs1, no[1]), pz = lift_point(k, p.vs2, no[2]);
    const int hc = min(p.crop_hw[b * 2 + 0], p.FH), wc = min(p.crop_hw[b * 2 + 1], p.FW);   // slice semantics (detectors/imvoxelnet.py:69): clamped to the map
    LiftPixel h;
    const bool ok = lift_project(p.proj + (size_t)b * 12, px, py, pz, hc, wc, h);
    if (ok) off = ((b * p.FH + (int)h.yr) * p.FW + (int)h.xr);
    p.valid[(size_t)b * p.N + n] = ok ? 1 : 0;
  }
  const int nvox = (p.N - n0) < lpv ? (int)(p.N - n0) : lpv;   // group-uniform; <= 0 for groups past the end
  float *dst0 = p.volume + ((size_t)b * p.N + n0) * p.C;
  float vmax = 0.f;      // max |value stored| (ivx_backproject_mean_fwd_amax: the first neck layer's operand scale needs max |volume|)
  for (int s = 0; s < lpv; ++s) {
    const int o = __shfl(off, gbase + s, 64);
    if (s >= nvox) continue;
    const float *src = p.feat + (size_t)(o < 0 ? 0 : o) * p.C;
    for (int ch = g; ch < p.nchunk; ch += lpv) {
      if constexpr (VEC == 4) {
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (o >= 0) x = *reinterpret_cast<const f32x4 *>(src + ch * 4);
        *reinterpret_cast<f32x4 *>(dst0 + (size_t)s * p.C + ch * 4) = x;
        vmax = fmaxf(fmaxf(vmax, fmaxf(fabsf(x[0]), fabsf(x[1]))), fmaxf(fabsf(x[2]), fabsf(x[3])));
      } else {
        const float x = o >= 0 ? src[ch] : 0.f;
        dst0[(size_t)s * p.C + ch] = x;
        vmax = fmaxf(vmax, fabsf(x));
      }
    }
  }
  if (p.pmax) {          // (uniform) every lane of the workgroup gets here
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
    __shared__ float wmax[4];
    if (lane == 0) wmax[threadIdx.x >> 6] = vmax;
    __syncthreads();
    if (threadIdx.x == 0) p.pmax[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  }
}

// ------------------------------------------------------------------ host: one call path for every lift export
// A/B knob of the block order (default 0: workgroups in plain voxel order; IVX_BP_ORDER=1: XCD-contiguous eighths, see the kernel)
static int bp_q(int nblk) {
  static const int xcd_order = getenv("IVX_BP_ORDER") ? atoi(getenv("IVX_BP_ORDER")) : 0;
  return xcd_order ? (nblk + 7) / 8 : 0;
}

// One lift call as every export states it: bp_run validates it, fills the kernel's parameters and launches the one kernel the table selects.
struct BpCall {
  const char *what;                 // the export the caller called, for messages
  const ivx_backproject_desc *d;    // dims, feat_dtype, mode, sampling, first (the older exports build one; its voxel_size is not read)
  const float *voxel_size;          // host float[3]: the older exports' argument, d->voxel_size of a descriptor call
  const void *feat;                 // [B*V, FH, FW, C]; gathered: the pool [S, FH, FW, C]
  const float *proj;                // [B, V, 12];       gathered: the pool [S, 12]
  const float *new_origin;
  const int32_t *crop_hw;
  void *volume;
  int32_t *count;
  void *mean_out;
  uint8_t *valid;
  ivx_stream_t stream;
  float *partials = nullptr;        // ivx_backproject_mean_fwd_amax
  bool gather = false;              // ivx_backproject_gather_fwd: view_slot [B, V] lists slots of the S-slot pools
  const int32_t *view_slot = nullptr;
  int32_t S = 0;
  bool listed = false;              // ivx_backproject_lists_fwd: the gathered form (gather is set too) with the row / first lists of `lists`
  const ivx_lift_lists *lists = nullptr;
  bool weighted = false;            // ivx_backproject_weighted_fwd: the listed form (listed and gather are set too) with the weights, decays and weight sums of `weights`
  const ivx_lift_weights *weights = nullptr;
  bool mapped = false;              // ivx_backproject_mapped_fwd with at least one map: the weighted form (weighted, listed and gather are set too) with the maps and the gate of `maps`
  const ivx_lift_maps *maps = nullptr;
};

// The descriptor of an older export's argument list (voxel_size stays with the caller's pointer, which may be NULL until validated).
static ivx_backproject_desc bp_desc(int32_t B, int32_t V, int32_t FH, int32_t FW, int32_t C, int32_t X, int32_t Y, int32_t Z, int32_t feat_dtype, int32_t mode,
                                    int32_t first = 0) {
  return ivx_backproject_desc{B, V, FH, FW, C, X, Y, Z, {0.f, 0.f, 0.f}, feat_dtype, mode, IVX_SAMPLE_NEAREST, first};
}

// The nearest fp32 mean of ONE view is a bit copy (keeps -0, denormals, bf16 pairs passed as words) and the only lift that writes per-workgroup maxima.
static bool bp_single_view_copy(const BpCall &c) {
  return !c.gather && c.d->sampling == IVX_SAMPLE_NEAREST && c.d->mode == IVX_LIFT_MEAN && c.d->feat_dtype == IVX_F32 && c.d->V == 1;
}

// What a lift accepts: IVX_ERR_INVALID_ARG with a message that names the export, before anything is launched or dereferenced.
static int bp_validate(const BpCall &c) {
  const char *what = c.what;
  const ivx_backproject_desc *d = c.d;
  IVX_REQUIRE(d, "%s: null descriptor", what);
  IVX_REQUIRE(d->sampling == IVX_SAMPLE_NEAREST || d->sampling == IVX_SAMPLE_BILINEAR, "%s: sampling %d (IVX_SAMPLE_NEAREST | IVX_SAMPLE_BILINEAR)", what, d->sampling);
  if (c.listed) {
    IVX_REQUIRE(c.lists, "%s: null lists", what);
    IVX_REQUIRE(d->mode == IVX_LIFT_MEAN || d->mode == IVX_LIFT_ACCUM, "%s: mode %d (IVX_LIFT_MEAN | IVX_LIFT_ACCUM: the sum mode has no listed form)", what, d->mode);
  } else if (c.gather) {
    IVX_REQUIRE(d->mode == IVX_LIFT_MEAN, "%s: mode %d (IVX_LIFT_MEAN only)", what, d->mode);
  }
  IVX_REQUIRE(d->mode == IVX_LIFT_MEAN || d->mode == IVX_LIFT_SUM || d->mode == IVX_LIFT_ACCUM, "%s: mode %d (IVX_LIFT_MEAN | IVX_LIFT_SUM | IVX_LIFT_ACCUM)", what, d->mode);
  IVX_REQUIRE(d->feat_dtype == IVX_F32 || d->feat_dtype == IVX_BF16, "%s: feat_dtype %d (IVX_F32 | IVX_BF16)", what, d->feat_dtype);
  IVX_REQUIRE(c.feat && c.proj && c.new_origin && c.crop_hw && c.voxel_size && c.volume && (!c.gather || c.view_slot), "%s: null argument", what);
  if (d->mode == IVX_LIFT_MEAN) {
    IVX_REQUIRE(c.valid, "%s: null argument (the mean mode writes valid)", what);
    IVX_REQUIRE(!c.count && !c.mean_out, "%s: the mean mode takes no count / mean_out", what);
  } else if (d->mode == IVX_LIFT_SUM) {
    IVX_REQUIRE(c.count, "%s: null argument (the sum mode writes count)", what);
    IVX_REQUIRE(!c.valid && !c.mean_out, "%s: the sum mode takes no valid / mean_out", what);
  } else {
    IVX_REQUIRE(c.count, "%s: null argument (the accumulate mode updates count)", what);
    IVX_REQUIRE((c.mean_out != nullptr) == (c.valid != nullptr), "%s: mean_out and valid must both be given or both be NULL", what);
  }
  if (c.gather) IVX_REQUIRE(c.S > 0, "%s: S=%d slots (the pools need at least one)", what, c.S);
  if (c.listed) {
    IVX_REQUIRE(c.lists->R > 0, "%s: R=%d rows (the state / output pools need at least one)", what, c.lists->R);
    IVX_REQUIRE(d->mode == IVX_LIFT_ACCUM || !c.lists->first, "%s: the mean mode takes no first list", what);
  }
  IVX_REQUIRE(d->B > 0 && d->V > 0 && d->FH > 0 && d->FW > 0 && d->C > 0 && d->X > 0 && d->Y > 0 && d->Z > 0, "%s: non-positive dims", what);
  if (c.listed) IVX_REQUIRE(c.lists->row || c.lists->R >= d->B, "%s: R=%d rows for B=%d samples and no row list (sample b then uses row b)", what, c.lists->R, d->B);
  if (c.weighted) {
    const ivx_lift_weights *w = c.weights;
    IVX_REQUIRE(w, "%s: null weights", what);
    IVX_REQUIRE(w->forget_below >= 0.f && w->forget_below < __builtin_inff(), "%s: forget_below %g (must be >= 0 and finite)", what, (double)w->forget_below);
    if (d->mode == IVX_LIFT_ACCUM) {
      IVX_REQUIRE(w->wsum, "%s: null wsum (the accumulate mode updates the weight sums)", what);
    } else {
      IVX_REQUIRE(!w->wsum, "%s: the mean mode takes no wsum", what);
      IVX_REQUIRE(!w->decay, "%s: the mean mode takes no decay list", what);
      IVX_REQUIRE(w->forget_below == 0.f, "%s: forget_below %g in the mean mode (must be 0: there is no state to forget)", what, (double)w->forget_below);
    }
  }
  if (c.mapped && c.maps->depth) {
    const ivx_lift_maps *m = c.maps;
    IVX_REQUIRE(m->behind >= 0.f && m->front >= 0.f, "%s: gate (behind %g, front %g): both must be >= 0 (+inf: no limit on that side), never NaN", what, (double)m->behind,
                (double)m->front);
  }
  const int vec = (d->C % 4 == 0) ? 4 : 1;
  IVX_REQUIRE(vec == 4 || (d->mode == IVX_LIFT_MEAN && d->feat_dtype == IVX_F32 && !c.gather), "%s: C %% 4 must be 0 (every form but the fp32 mean of a view stack)", what);
  IVX_REQUIRE((int64_t)d->X * d->Y * d->Z < (1LL << 31), "%s: voxel grid too large", what);
  if (c.gather) {
    IVX_REQUIRE((int64_t)c.S * d->FH * d->FW < (1LL << 31), "%s: feature pool too large", what);
    IVX_REQUIRE((int64_t)d->B * d->V < (1LL << 31), "%s: view list too large", what);
  } else {
    IVX_REQUIRE((int64_t)d->B * d->V * d->FH * d->FW < (1LL << 31), "%s: feature maps too large", what);
  }
  IVX_REQUIRE(d->B <= 65535, "%s: batch too large", what);
  IVX_REQUIRE((d->C + vec - 1) / vec <= 64 * 4, "%s: C=%d too large (max %d)", what, d->C, 256 * vec);
  IVX_REQUIRE(!c.partials || bp_single_view_copy(c), "%s: partial maxima come from the single-view kernel only", what);
  return IVX_OK;
}

// The kernel's parameters and grid of a validated call: the one place that writes a BpParams / BpGatherParams / BpListParams / BpWeightParams /
// BpMapParams (a plain, gathered, listed or weighted launch passes the base).
static BpMapParams bp_fill(const BpCall &c, dim3 *grid) {
  const ivx_backproject_desc &d = *c.d;
  BpMapParams p;
  p.feat = (const float *)c.feat; p.proj = c.proj; p.new_origin = c.new_origin; p.crop_hw = c.crop_hw;
  p.volume = (float *)c.volume; p.valid = c.valid; p.count = c.count; p.mean_out = c.mean_out;
  // the running state is read unless `first`; a bf16 sum is the accumulate kernel from a zero state (bp_launch), so it never reads one
  p.first = d.mode == IVX_LIFT_ACCUM ? d.first : (d.mode == IVX_LIFT_SUM && d.feat_dtype == IVX_BF16) ? 1 : 0;
  p.vs0 = c.voxel_size[0]; p.vs1 = c.voxel_size[1]; p.vs2 = c.voxel_size[2];
  p.V = d.V; p.FH = d.FH; p.FW = d.FW; p.C = d.C; p.X = d.X; p.Y = d.Y; p.Z = d.Z; p.N = d.X * d.Y * d.Z;
  const int vec = (d.C % 4 == 0) ? 4 : 1;
  p.nchunk = (d.C + vec - 1) / vec;
  int lg = 0;
  while ((1 << lg) < p.nchunk && lg < 6) ++lg;
  p.lpv_log2 = lg;
  p.view_slot = c.view_slot; p.S = c.S;
  p.row = c.listed ? c.lists->row : nullptr; p.first_list = c.listed ? c.lists->first : nullptr; p.R = c.listed ? c.lists->R : 0;
  p.view_weight = c.weighted ? c.weights->view_weight : nullptr; p.decay = c.weighted ? c.weights->decay : nullptr;
  p.forget_below = c.weighted ? c.weights->forget_below : 0.f; p.wsum = c.weighted ? c.weights->wsum : nullptr;
  p.pixel_weight = c.mapped ? c.maps->pixel_weight : nullptr; p.depth = c.mapped ? c.maps->depth : nullptr;
  p.behind = c.mapped && c.maps->depth ? c.maps->behind : 0.f; p.front = c.mapped && c.maps->depth ? c.maps->front : 0.f;
  if (bp_single_view_copy(c)) {      // 256 voxels per workgroup regardless of the group width (each lane projects one voxel)
    p.pmax = c.partials; p.nblk = 0; p.q = 0;
    *grid = dim3((p.N + 255) / 256, d.B);
    return p;
  }
  const int vox_per_block = 256 >> lg;
  p.pmax = nullptr; p.nblk = (p.N + vox_per_block - 1) / vox_per_block; p.q = bp_q(p.nblk);
  *grid = dim3(p.q ? 8u * (unsigned)p.q : (unsigned)p.nblk, d.B);
  return p;
}

// Both feature types of one VEC 4 form of the multi-view kernel: the helper of the table below for the forms that exist for float and __bf16.
template <int MODE, int SAMP, bool GATHER = false, bool ROWS = false, bool WEIGHTED = false, bool MAPPED = false, typename P>
static void bp_launch_t(const bool bf16, const dim3 grid, hipStream_t st, const P &p) {
  if (bf16) hipLaunchKernelGGL((backproject_mean_kernel<4, MODE, __bf16, SAMP, GATHER, ROWS, WEIGHTED, MAPPED>), grid, dim3(256), 0, st, p);
  else      hipLaunchKernelGGL((backproject_mean_kernel<4, MODE, float, SAMP, GATHER, ROWS, WEIGHTED, MAPPED>), grid, dim3(256), 0, st, p);
}

// The selection table: every instantiation of the two lift kernels is launched from exactly one line below (a bp_launch_t line: both types).
static int bp_launch(const BpCall &c, const BpMapParams &m, const dim3 grid) {
  const ivx_backproject_desc &d = *c.d;
  const BpWeightParams &w = m;
  const BpListParams &l = w;
  const BpGatherParams &g = l;
  const BpParams &p = l;
  const bool bf16 = d.feat_dtype == IVX_BF16, bilinear = d.sampling == IVX_SAMPLE_BILINEAR, vec4 = d.C % 4 == 0;
  // BP_SUM exists for fp32 features only: a bf16 sum runs BP_ACCUM (fp32 sums) with first = 1 and no mean_out (bp_fill, bp_validate)
  const int mode = d.mode == IVX_LIFT_MEAN ? BP_MEAN : (d.mode == IVX_LIFT_SUM && !bf16) ? BP_SUM : BP_ACCUM;
  const dim3 block(256);
  hipStream_t st = (hipStream_t)c.stream;
  if (c.mapped) {                                   // pixel maps: the WEIGHTED forms with a confidence and / or a gated depth per pixel
    if (mode == BP_ACCUM && bilinear)  bp_launch_t<BP_ACCUM, BP_BILINEAR, true, true, true, true>(bf16, grid, st, m);
    else if (mode == BP_ACCUM)         bp_launch_t<BP_ACCUM, BP_NEAREST, true, true, true, true>(bf16, grid, st, m);
    else if (bilinear)                 bp_launch_t<BP_MEAN, BP_BILINEAR, true, true, true, true>(bf16, grid, st, m);
    else                               bp_launch_t<BP_MEAN, BP_NEAREST, true, true, true, true>(bf16, grid, st, m);
  } else if (c.weighted) {                          // weights, decay and weight sums: the ROWS forms, with or without a row list
    if (mode == BP_ACCUM && bilinear)  bp_launch_t<BP_ACCUM, BP_BILINEAR, true, true, true>(bf16, grid, st, w);
    else if (mode == BP_ACCUM)         bp_launch_t<BP_ACCUM, BP_NEAREST, true, true, true>(bf16, grid, st, w);
    else if (bilinear)                 bp_launch_t<BP_MEAN, BP_BILINEAR, true, true, true>(bf16, grid, st, w);
    else                               bp_launch_t<BP_MEAN, BP_NEAREST, true, true, true>(bf16, grid, st, w);
  } else if (c.listed && (mode == BP_ACCUM || l.row)) {    // rows of a state / output pool: MEAN and ACCUM, VEC 4 only (a listed mean with no row list is the gathered launch below)
    if (mode == BP_ACCUM && bilinear)  bp_launch_t<BP_ACCUM, BP_BILINEAR, true, true>(bf16, grid, st, l);
    else if (mode == BP_ACCUM)         bp_launch_t<BP_ACCUM, BP_NEAREST, true, true>(bf16, grid, st, l);
    else if (bilinear)                 bp_launch_t<BP_MEAN, BP_BILINEAR, true, true>(bf16, grid, st, l);
    else                               bp_launch_t<BP_MEAN, BP_NEAREST, true, true>(bf16, grid, st, l);
  } else if (c.gather) {                            // MEAN only, VEC 4 only, one listed view too
    if (bilinear)  bp_launch_t<BP_MEAN, BP_BILINEAR, true>(bf16, grid, st, g);
    else           bp_launch_t<BP_MEAN, BP_NEAREST, true>(bf16, grid, st, g);
  } else if (bilinear) {                            // one view too: the blend is arithmetic, not a copy
    if (mode == BP_MEAN && vec4)  bp_launch_t<BP_MEAN, BP_BILINEAR>(bf16, grid, st, p);
    else if (mode == BP_MEAN)     hipLaunchKernelGGL((backproject_mean_kernel<1, BP_MEAN, float, BP_BILINEAR>), grid, block, 0, st, p);
    else if (mode == BP_SUM)      hipLaunchKernelGGL((backproject_mean_kernel<4, BP_SUM, float, BP_BILINEAR>), grid, block, 0, st, p);
    else                          bp_launch_t<BP_ACCUM, BP_BILINEAR>(bf16, grid, st, p);
  } else if (bp_single_view_copy(c)) {              // nearest fp32 mean of one view: the copy kernel (a bf16 view is not: its mean converts)
    if (vec4)  hipLaunchKernelGGL(backproject_single_view_kernel<4>, grid, block, 0, st, p);
    else       hipLaunchKernelGGL(backproject_single_view_kernel<1>, grid, block, 0, st, p);
  } else {
    if (mode == BP_MEAN && vec4)  bp_launch_t<BP_MEAN, BP_NEAREST>(bf16, grid, st, p);
    else if (mode == BP_MEAN)     hipLaunchKernelGGL(backproject_mean_kernel<1>, grid, block, 0, st, p);
    else if (mode == BP_SUM)      hipLaunchKernelGGL((backproject_mean_kernel<4, BP_SUM>), grid, block, 0, st, p);
    else                          bp_launch_t<BP_ACCUM, BP_NEAREST>(bf16, grid, st, p);
  }
  IVX_CHECK_LAUNCH(c.what);
  return IVX_OK;
}

static int bp_run(const BpCall &c) {
  const int rc = bp_validate(c);
  if (rc != IVX_OK) return rc;
  dim3 grid;
  return bp_launch(c, bp_fill(c, &grid), grid);
}

// ------------------------------------------------------------------ the exports (include/imvoxel.h): each states its call and runs it
extern "C" int ivx_backproject_mean_fwd(const float *feat, int32_t B, int32_t V, int32_t FH, int32_t FW, int32_t C,
                                        const float *proj, const float *new_origin, const int32_t *crop_hw,
                                        const float *voxel_size, int32_t X, int32_t Y, int32_t Z, float *volume,
                                        uint8_t *valid, ivx_stream_t stream) {
  const ivx_backproject_desc d = bp_desc(B, V, FH, FW, C, X, Y, Z, IVX_F32, IVX_LIFT_MEAN);
  return bp_run({"ivx_backproject_mean_fwd", &d, voxel_size, feat, proj, new_origin, crop_hw, volume, nullptr, nullptr, valid, stream});
}

// Single-view lift that also leaves one max |volume| per workgroup: ivx_backproject_amax_blocks(B, V, X, Y, Z) floats (0: this shape
// takes the multi-view kernel, which does not -- the consumer reduces the volume itself), for ivx_conv_winograd_input_amax.
extern "C" int32_t ivx_backproject_amax_blocks(int32_t B, int32_t V, int32_t X, int32_t Y, int32_t Z) {
  if (B <= 0 || V != 1 || X <= 0 || Y <= 0 || Z <= 0 || (int64_t)X * Y * Z >= (1LL << 31)) return 0;
  return (int32_t)(((int64_t)X * Y * Z + 255) / 256 * B);
}

extern "C" int ivx_backproject_mean_fwd_amax(const float *feat, int32_t B, int32_t V, int32_t FH, int32_t FW, int32_t C, const float *proj,
                                             const float *new_origin, const int32_t *crop_hw, const float *voxel_size, int32_t X, int32_t Y,
                                             int32_t Z, float *volume, uint8_t *valid, float *partials, ivx_stream_t stream) {
  const ivx_backproject_desc d = bp_desc(B, V, FH, FW, C, X, Y, Z, IVX_F32, IVX_LIFT_MEAN);
  return bp_run({"ivx_backproject_mean_fwd_amax", &d, voxel_size, feat, proj, new_origin, crop_hw, volume, nullptr, nullptr, valid, stream, partials});
}

// bf16 storage (optional reduced-precision mode): feat / volume are bf16, everything else as ivx_backproject_mean_fwd.  One view runs the
// mean kernel here too; callers that want the copy pass the bf16 map as C/2 32-bit words to ivx_backproject_mean_fwd.  C % 4 == 0.
extern "C" int ivx_backproject_mean_fwd_bf16(const void *feat, int32_t B, int32_t V, int32_t FH, int32_t FW, int32_t C,
                                             const float *proj, const float *new_origin, const int32_t *crop_hw,
                                             const float *voxel_size, int32_t X, int32_t Y, int32_t Z, void *volume,
                                             uint8_t *valid, ivx_stream_t stream) {
  const ivx_backproject_desc d = bp_desc(B, V, FH, FW, C, X, Y, Z, IVX_BF16, IVX_LIFT_MEAN);
  return bp_run({"ivx_backproject_mean_fwd_bf16", &d, voxel_size, feat, proj, new_origin, crop_hw, volume, nullptr, nullptr, valid, stream});
}

extern "C" int ivx_backproject_sum_fwd(const float *feat, int32_t B, int32_t V, int32_t FH, int32_t FW, int32_t C,
                                       const float *proj, const float *new_origin, const int32_t *crop_hw,
                                       const float *voxel_size, int32_t X, int32_t Y, int32_t Z, float *volume_sum,
                                       int32_t *count, ivx_stream_t stream) {
  const ivx_backproject_desc d = bp_desc(B, V, FH, FW, C, X, Y, Z, IVX_F32, IVX_LIFT_SUM);
  return bp_run({"ivx_backproject_sum_fwd", &d, voxel_size, feat, proj, new_origin, crop_hw, volume_sum, count, nullptr, nullptr, stream});
}

// Streaming scenes: add V views to a running (sum, count) volume (BP_ACCUM mode of backproject_mean_kernel).
extern "C" int ivx_backproject_accum_fwd(const float *feat, int32_t B, int32_t V, int32_t FH, int32_t FW, int32_t C, const float *proj,
                                         const float *new_origin, const int32_t *crop_hw, const float *voxel_size, int32_t X, int32_t Y,
                                         int32_t Z, float *volume_sum, int32_t *count, int32_t first, float *mean_out, uint8_t *valid_out,
                                         ivx_stream_t stream) {
  const ivx_backproject_desc d = bp_desc(B, V, FH, FW, C, X, Y, Z, IVX_F32, IVX_LIFT_ACCUM, first);
  return bp_run({"ivx_backproject_accum_fwd", &d, voxel_size, feat, proj, new_origin, crop_hw, volume_sum, count, mean_out, valid_out, stream});
}

extern "C" int ivx_backproject_accum_fwd_bf16(const void *feat, int32_t B, int32_t V, int32_t FH, int32_t FW, int32_t C, const float *proj,
                                              const float *new_origin, const int32_t *crop_hw, const float *voxel_size, int32_t X, int32_t Y,
                                              int32_t Z, float *volume_sum, int32_t *count, int32_t first, void *mean_out, uint8_t *valid_out,
                                              ivx_stream_t stream) {
  const ivx_backproject_desc d = bp_desc(B, V, FH, FW, C, X, Y, Z, IVX_BF16, IVX_LIFT_ACCUM, first);
  return bp_run({"ivx_backproject_accum_fwd_bf16", &d, voxel_size, feat, proj, new_origin, crop_hw, volume_sum, count, mean_out, valid_out, stream});
}

// One entry point for both sampling rules, the three modes and both feature types (include/imvoxel.h).
extern "C" int ivx_backproject_fwd_ex(const ivx_backproject_desc *d, const void *feat, const float *proj, const float *new_origin,
                                      const int32_t *crop_hw, void *volume, int32_t *count, void *mean_out, uint8_t *valid, ivx_stream_t stream) {
  return bp_run({"ivx_backproject_fwd_ex", d, d ? d->voxel_size : nullptr, feat, proj, new_origin, crop_hw, volume, count, mean_out, valid, stream});
}

// Gathered mean lift (include/imvoxel.h): the listed views of a feature / projection pool, in list order.
extern "C" int ivx_backproject_gather_fwd(const ivx_backproject_desc *d, int32_t S, const void *feat_pool, const float *proj_pool, const int32_t *view_slot,
                                          const float *new_origin, const int32_t *crop_hw, void *volume, uint8_t *valid, ivx_stream_t stream) {
  return bp_run({"ivx_backproject_gather_fwd", d, d ? d->voxel_size : nullptr, feat_pool, proj_pool, new_origin, crop_hw, volume, nullptr, nullptr, valid, stream,
                 nullptr, true, view_slot, S});
}

// Listed lift with per-sample state (include/imvoxel.h): the gathered form whose samples name their rows of the state / output pools.
extern "C" int ivx_backproject_lists_fwd(const ivx_backproject_desc *d, const ivx_lift_lists *l, const void *feat_pool, const float *proj_pool,
                                         const float *new_origin, const int32_t *crop_hw, void *volume, int32_t *count, void *mean_out, uint8_t *valid,
                                         ivx_stream_t stream) {
  return bp_run({"ivx_backproject_lists_fwd", d, d ? d->voxel_size : nullptr, feat_pool, proj_pool, new_origin, crop_hw, volume, count, mean_out, valid, stream,
                 nullptr, true, l ? l->view_slot : nullptr, l ? l->S : 0, true, l});
}

// Weighted listed lift (include/imvoxel.h): the listed form with per-view weights, a per-sample decay and the weight sums beside the counts.
extern "C" int ivx_backproject_weighted_fwd(const ivx_backproject_desc *d, const ivx_lift_lists *l, const ivx_lift_weights *w, const void *feat_pool,
                                            const float *proj_pool, const float *new_origin, const int32_t *crop_hw, void *volume, int32_t *count, void *mean_out,
                                            uint8_t *valid, ivx_stream_t stream) {
  return bp_run({"ivx_backproject_weighted_fwd", d, d ? d->voxel_size : nullptr, feat_pool, proj_pool, new_origin, crop_hw, volume, count, mean_out, valid, stream,
                 nullptr, true, l ? l->view_slot : nullptr, l ? l->S : 0, true, l, true, w});
}

// Weighted listed lift with pixel maps (include/imvoxel.h): per view a confidence per pixel and / or a depth map with a gate.  No map: the weighted entry's launch.
extern "C" int ivx_backproject_mapped_fwd(const ivx_backproject_desc *d, const ivx_lift_lists *l, const ivx_lift_weights *w, const ivx_lift_maps *m,
                                          const void *feat_pool, const float *proj_pool, const float *new_origin, const int32_t *crop_hw, void *volume,
                                          int32_t *count, void *mean_out, uint8_t *valid, ivx_stream_t stream) {
  const bool mapped = m && (m->pixel_weight || m->depth);
  return bp_run({"ivx_backproject_mapped_fwd", d, d ? d->voxel_size : nullptr, feat_pool, proj_pool, new_origin, crop_hw, volume, count, mean_out, valid, stream,
                 nullptr, true, l ? l->view_slot : nullptr, l ? l->S : 0, true, l, true, w, mapped, mapped ? m : nullptr});
}

// ------------------------------------------------------------------ mean of a (sum, count) or (sum, weight sum) volume
// out == sum: in place (ivx_volume_normalize_fwd).  Otherwise the sums stay intact and out may be bf16 (ivx_volume_mean_fwd, ivx_volume_wmean_fwd).
template <typename E>
static int volume_normalize_launch(const char *what, const float *sum, void *out, int32_t out_dtype, const E *evidence, int64_t n_voxels, int32_t C,
                                   uint8_t *valid, ivx_stream_t stream) {
  IVX_REQUIRE(n_voxels > 0 && C > 0 && C % 4 == 0, "%s: bad dims (C %% 4 must be 0)", what);
  IVX_REQUIRE(out_dtype == IVX_F32 || out_dtype == IVX_BF16, "%s: out_dtype must be IVX_F32 or IVX_BF16", what);
  const long long total4 = (long long)n_voxels * (C / 4);
  long long blocks = (total4 + 255) / 256;
  if (blocks > 256 * 64) blocks = 256 * 64;
  if (out_dtype == IVX_BF16)
    hipLaunchKernelGGL((volume_normalize_kernel<__bf16, E>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, sum, (__bf16 *)out, evidence, valid, total4, C / 4);
  else
    hipLaunchKernelGGL((volume_normalize_kernel<float, E>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, sum, (float *)out, evidence, valid, total4, C / 4);
  IVX_CHECK_LAUNCH(what);
  return IVX_OK;
}

extern "C" int ivx_volume_normalize_fwd(float *volume, const int32_t *count, int64_t n_voxels, int32_t C, uint8_t *valid,
                                        ivx_stream_t stream) {
  IVX_REQUIRE(volume && count && valid, "ivx_volume_normalize_fwd: null argument");
  return volume_normalize_launch("ivx_volume_normalize_fwd", volume, volume, IVX_F32, count, n_voxels, C, valid, stream);
}

extern "C" int ivx_volume_mean_fwd(const float *volume_sum, const int32_t *count, int64_t n_voxels, int32_t C, void *out, int32_t out_dtype,
                                   uint8_t *valid, ivx_stream_t stream) {
  IVX_REQUIRE(volume_sum && count && out && valid, "ivx_volume_mean_fwd: null argument");
  IVX_REQUIRE((const void *)volume_sum != out, "ivx_volume_mean_fwd: out must not be volume_sum (ivx_volume_normalize_fwd works in place)");
  return volume_normalize_launch("ivx_volume_mean_fwd", volume_sum, out, out_dtype, count, n_voxels, C, valid, stream);
}

extern "C" int ivx_volume_wmean_fwd(const float *volume_sum, const float *wsum, int64_t n_voxels, int32_t C, void *out, int32_t out_dtype, uint8_t *valid,
                                    ivx_stream_t stream) {
  const char *what = "ivx_volume_wmean_fwd";
  IVX_REQUIRE(volume_sum && wsum && out && valid, "%s: null argument", what);
  IVX_REQUIRE((const void *)volume_sum != out, "%s: out must not be volume_sum", what);
  return volume_normalize_launch(what, volume_sum, out, out_dtype, wsum, n_voxels, C, valid, stream);
}
