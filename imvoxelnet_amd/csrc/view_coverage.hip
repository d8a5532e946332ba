// View coverage (ivx_view_coverage_fwd, include/imvoxel.h): per candidate view of a scene, the number of voxels the lift would count the view
// at, and the number of those for which the scene holds less than `fresh_below` of evidence.  A keyframe gate asks it before the 2-D trunk runs
// (scene.py, SceneSession.coverage / add_views(..., min_novelty=)).  Nothing but the [B,V,2] int32 result is written.
//
// Work split.  One lane owns one voxel, consecutive lanes consecutive n, so the one state read per voxel (4 bytes of count / wsum, 1 byte of
// the mask) is coalesced and happens once however many candidates there are.  The candidate loop runs inside the lane: for candidate v every
// lane projects ITS voxel by the rows of slot view_slot[b*V + v].  blockIdx.y is the sample, so the slot, the twelve projection numbers, the
// row, the origin and the crop are uniform over the workgroup and are indexed by uniform values only: the compiler keeps them in scalar
// registers (scalar loads; the per-lane arithmetic takes them as scalar operands).
//
// Counting.  Per candidate a 64-bit __ballot of `sees` and of `sees && fresh` and two __popcll give the wave's two counts; lane 0 of the wave
// adds them to the workgroup's counters in LDS (integer LDS atomics, 2 * V words), over all the voxel blocks the workgroup walks; after one
// barrier the workgroup issues at most ONE global integer atomicAdd per (candidate, counter), and none for a zero.  Integer atomics only: the
// sum does not depend on the order of arrival, so the result is pinned with == (tests/test_gpu_view_coverage.py).  The entry zeroes `out` on
// the stream before the launch.
//
// Shape.  A grid-stride loop over blocks of IVX_COVERAGE_WG voxels; gridDim.x = min(voxel blocks, IVX_COVERAGE_WGS / B), so the number of
// workgroups of a launch stays near a small multiple of the CU count and the global atomics per launch stay at most 2 * V * that many.
// IVX_COVERAGE_WGS is read from the environment at every call (default below; the tests lower it to walk the stride loop at a small grid).
// Tried (profiles/view_coverage.md, section (b); bare calls, a memset and a kernel each): the call takes 10.6 - 11.5 us for one candidate on the
// ScanNet-fast AND the ScanNet-v1 grid against 7.7 us for two tiny launches -- launch latency, not the 0.1 / 0.8 MB of state -- and 15.2 us for 8
// candidates at ScanNet v1, where the candidate loop's arithmetic shows.  Caps of 256, 1024 and 4096 workgroups measure alike (15.2 us); 64 are too
// few (39.4 us).  128 and 64 lanes per workgroup lose at ScanNet v1 (18.3 and 24.0 against 15.3 us at 8 candidates: more workgroups, more global
// atomics) and tie on the small grid.  Adopted: 256 lanes, cap 1024.
//
// Arithmetic: csrc/lift_geometry.h, the lift's chain; compiled with -ffp-contract=off like backproject.hip.
#include <stdlib.h>

#include <algorithm>

#include "ivx_common.h"
#include "lift_geometry.h"

#ifndef IVX_COVERAGE_WG
#define IVX_COVERAGE_WG 256
#endif
#ifndef IVX_COVERAGE_WGS_DEFAULT
#define IVX_COVERAGE_WGS_DEFAULT 1024
#endif

namespace {

constexpr int COV_MAX_V = 256;     // candidates per sample: the LDS counters are 2 * COV_MAX_V words

struct CovParams {
  const float *proj_pool;     // [S, 12]
  const int *view_slot;       // [B, V]
  const int *row;             // [B] or NULL (= b)
  const float *new_origin;    // [B, 3]
  const int *crop_hw;         // [B, 2]
  const void *state;          // [R, N] int32 / fp32 / uint8 by KIND, or NULL
  const float *pixel_weight;  // [S, FH, FW] or NULL
  const float *depth;         // [S, FH, FW] or NULL
  int *out;                   // [B, V, 2]
  float vs0, vs1, vs2;
  float behind, front, fresh_below;
  int V, S, R, FH, FW, Y, Z, N;
  int nblk;                   // voxel blocks per sample
};

// den(b, n): the evidence the scene holds at voxel n of row r.
template <int KIND>
__device__ __forceinline__ float cov_den(const void *state, const size_t at) {
  if constexpr (KIND == IVX_STATE_COUNT) return (float)reinterpret_cast<const int32_t *>(state)[at];
  if constexpr (KIND == IVX_STATE_WSUM) return reinterpret_cast<const float *>(state)[at];
  if constexpr (KIND == IVX_STATE_MASK) return reinterpret_cast<const uint8_t *>(state)[at] ? 1.0f : 0.0f;
  return 0.0f;
}

template <int KIND>
__global__ __launch_bounds__(IVX_COVERAGE_WG) void view_coverage_kernel(const CovParams p) {
  __shared__ int acc[2 * COV_MAX_V];
  const int b = blockIdx.y;
  const int r = p.row ? p.row[b] : b;
  if (r < 0 || r >= p.R) return;                 // (uniform: r depends on blockIdx.y alone, so no lane stays behind at the barriers below)
  for (int i = threadIdx.x; i < 2 * p.V; i += IVX_COVERAGE_WG) acc[i] = 0;
  __syncthreads();
  const float *no = p.new_origin + b * 3;
  const float o0 = no[0], o1 = no[1], o2 = no[2];
  const int hc = min(p.crop_hw[b * 2 + 0], p.FH), wc = min(p.crop_hw[b * 2 + 1], p.FW);     // the lift's slice semantics: clamped to the map
  const int *slots = p.view_slot + b * p.V;
  const int lane = threadIdx.x & 63;

  for (int blk = blockIdx.x; blk < p.nblk; blk += gridDim.x) {     // (uniform per workgroup: whole waves reach every ballot)
    const int n = blk * IVX_COVERAGE_WG + (int)threadIdx.x;
    const bool active = n < p.N;
    const int nn = active ? n : p.N - 1;
    int i, j, k;
    lift_voxel(nn, p.Y, p.Z, i, j, k);
    const float px = lift_point(i, p.vs0, o0), py = lift_point(j, p.vs1, o1), pz = lift_point(k, p.vs2, o2);
    const float den = cov_den<KIND>(p.state, (size_t)r * p.N + nn);
    const bool fresh = !(den >= p.fresh_below);  // a NaN evidence is fresh; equality is not
    for (int v = 0; v < p.V; ++v) {
      const int slot = slots[v];                 // uniform
      if (slot < 0 || slot >= p.S) continue;     // a padded or unknown slot sees nothing: no address of it is formed
      LiftPixel h;
      bool ok = active && lift_project(p.proj_pool + (size_t)slot * 12, px, py, pz, hc, wc, h);
      if (ok && (p.depth || p.pixel_weight)) {   // inside the crop, hence inside the map: (int)yr in [0, FH), (int)xr in [0, FW), slot in [0, S)
        const int pix = (slot * p.FH + (int)h.yr) * p.FW + (int)h.xr;
        const float D = p.depth ? p.depth[pix] : 0.f;
        const float pw = p.pixel_weight ? p.pixel_weight[pix] : 1.0f;
        ok = lift_gate(D, h.d, p.behind, p.front) && lift_weight_counts(pw);
      }
      const unsigned long long seen = __ballot(ok), novel = __ballot(ok && fresh);
      if (lane == 0 && seen) {
        atomicAdd(&acc[2 * v], __popcll(seen));
        if (novel) atomicAdd(&acc[2 * v + 1], __popcll(novel));
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * p.V; i += IVX_COVERAGE_WG) {
    const int c = acc[i];
    if (c) atomicAdd(p.out + (size_t)b * 2 * p.V + i, c);
  }
}

}  // namespace

extern "C" int ivx_view_coverage_fwd(const ivx_backproject_desc *d, const ivx_lift_lists *l, const ivx_lift_maps *m, const float *proj_pool,
                                     const float *new_origin, const int32_t *crop_hw, const void *state, int32_t state_kind, float fresh_below, int32_t *out,
                                     ivx_stream_t stream) {
  const char *what = "ivx_view_coverage_fwd";
  IVX_REQUIRE(d, "%s: null descriptor", what);
  IVX_REQUIRE(l, "%s: null lists", what);
  IVX_REQUIRE(proj_pool && l->view_slot && new_origin && crop_hw && out, "%s: null argument (proj_pool, view_slot, new_origin, crop_hw and out are required)", what);
  IVX_REQUIRE(d->B > 0 && d->V > 0 && l->S > 0 && l->R > 0 && d->FH > 0 && d->FW > 0 && d->X > 0 && d->Y > 0 && d->Z > 0,
              "%s: non-positive dims (B, V, S, R, FH, FW, X, Y and Z must be positive)", what);
  IVX_REQUIRE((int64_t)d->X * d->Y * d->Z < (1LL << 31), "%s: voxel grid too large", what);
  IVX_REQUIRE((int64_t)l->S * d->FH * d->FW < (1LL << 31), "%s: map pool too large", what);
  IVX_REQUIRE((int64_t)d->B * d->V < (1LL << 31), "%s: view list too large", what);
  IVX_REQUIRE(d->B <= 65535, "%s: batch too large", what);
  IVX_REQUIRE(d->V <= COV_MAX_V, "%s: V=%d candidates per sample (max %d)", what, d->V, COV_MAX_V);
  IVX_REQUIRE(l->row || l->R >= d->B, "%s: R=%d rows for B=%d samples and no row list (sample b then uses row b)", what, l->R, d->B);
  IVX_REQUIRE(state_kind == IVX_STATE_NONE || state_kind == IVX_STATE_COUNT || state_kind == IVX_STATE_WSUM || state_kind == IVX_STATE_MASK,
              "%s: state_kind %d (IVX_STATE_NONE | IVX_STATE_COUNT | IVX_STATE_WSUM | IVX_STATE_MASK)", what, state_kind);
  IVX_REQUIRE((state != nullptr) == (state_kind != IVX_STATE_NONE), "%s: state and state_kind %d contradict each other (NULL goes with IVX_STATE_NONE alone)", what,
              state_kind);
  IVX_REQUIRE(fresh_below > 0.f && fresh_below < __builtin_inff(), "%s: fresh_below %g (must be > 0 and finite)", what, (double)fresh_below);
  IVX_REQUIRE(!l->first, "%s: takes no first list (nothing is accumulated)", what);
  const bool gated = m && m->depth;
  if (gated)
    IVX_REQUIRE(m->behind >= 0.f && m->front >= 0.f, "%s: gate (behind %g, front %g): both must be >= 0 (+inf: no limit on that side), never NaN", what, (double)m->behind,
                (double)m->front);

  CovParams p;
  p.proj_pool = proj_pool; p.view_slot = l->view_slot; p.row = l->row; p.new_origin = new_origin; p.crop_hw = crop_hw; p.state = state;
  p.pixel_weight = m ? m->pixel_weight : nullptr; p.depth = m ? m->depth : nullptr; p.out = out;
  p.vs0 = d->voxel_size[0]; p.vs1 = d->voxel_size[1]; p.vs2 = d->voxel_size[2];
  p.behind = gated ? m->behind : 0.f; p.front = gated ? m->front : 0.f; p.fresh_below = fresh_below;
  p.V = d->V; p.S = l->S; p.R = l->R; p.FH = d->FH; p.FW = d->FW; p.Y = d->Y; p.Z = d->Z; p.N = d->X * d->Y * d->Z;
  p.nblk = (p.N + IVX_COVERAGE_WG - 1) / IVX_COVERAGE_WG;
  const char *env = getenv("IVX_COVERAGE_WGS");
  int wgs = env ? atoi(env) : IVX_COVERAGE_WGS_DEFAULT;
  if (wgs < 1) wgs = IVX_COVERAGE_WGS_DEFAULT;
  const int gx = std::max(1, std::min(p.nblk, wgs / d->B));
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(out, 0, (size_t)d->B * d->V * 2 * sizeof(int32_t), st);
  if (e != hipSuccess) {
    ivx_set_error("%s: hipMemsetAsync failed: %s", what, hipGetErrorString(e));
    return IVX_ERR_HIP;
  }
  const dim3 grid((unsigned)gx, (unsigned)d->B), block(IVX_COVERAGE_WG);
  switch (state_kind) {
    case IVX_STATE_COUNT: hipLaunchKernelGGL(view_coverage_kernel<IVX_STATE_COUNT>, grid, block, 0, st, p); break;
    case IVX_STATE_WSUM:  hipLaunchKernelGGL(view_coverage_kernel<IVX_STATE_WSUM>, grid, block, 0, st, p); break;
    case IVX_STATE_MASK:  hipLaunchKernelGGL(view_coverage_kernel<IVX_STATE_MASK>, grid, block, 0, st, p); break;
    default:              hipLaunchKernelGGL(view_coverage_kernel<IVX_STATE_NONE>, grid, block, 0, st, p); break;
  }
  IVX_CHECK_LAUNCH(what);
  return IVX_OK;
}
