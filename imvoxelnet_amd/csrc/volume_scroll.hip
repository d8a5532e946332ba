// In-place voxel shift of rows of the scene state pools (ivx_volume_scroll_fwd, include/imvoxel.h): scrolling scenes, scene.py.
//
//   new[i,j,k] = old[i+sx, j+sy, k+sz]  where that source lies inside the grid, an unseen voxel (all bits zero) everywhere else,
//
// for the three state fields of a row: volume_sum [R,X,Y,Z,C] fp32 moved as 16-byte words, count [R,X,Y,Z] int32 and wsum [R,X,Y,Z] fp32 moved
// as 4-byte words.  No float arithmetic touches a value, so every bit pattern survives (NaN payloads, -0, denormals).
//
// One pass per axis with a non-zero shift, in the order x, y, z (each pass is the definition with the other two shifts zero, and those three
// maps commute: the order only fixes which launches run first).  In the pass along an axis of length L a row is [outer, L, inner] elements and
// ONE LANE OWNS ONE LINE (outer, inner); consecutive lanes take consecutive `inner`, so on the x and y passes a wave's loads and stores are
// contiguous (on the z pass of the sums a wave covers 64 / (C/4) whole voxels; on the z pass of count / wsum a lane's line is Z consecutive
// words and the wave strides by Z words -- 4 bytes per voxel, the small fields).
//
// Why in place is safe, with no scratch, no atomics and no barrier.  The lane walks its line in the direction of the shift (ascending for
// s > 0, descending for s < 0).  At walk step q it writes the q-th position of the walk and reads the (q + |s|)-th, or takes zero when that lies
// beyond the end of the line.  So the read position is always AHEAD of the write position in walk order: nothing that has been stored is
// ever read again, and no other lane touches the line.  The walk is unrolled by U: a block loads the U positions q .. q+U-1 (+|s|), then
// stores the U.  The next block's loads start at q+U+|s|, beyond everything stored so far, and inside a block every load precedes every store
// in program order (same lane, possibly the same address: program order holds).  That is the whole argument; it needs |s| >= 1 only.
// |s| >= L reads nothing and stores zeros: the row becomes all zero.
//
// U (IVX_SCROLL_U) keeps U independent loads in flight per lane: the ScanNet-fast x pass has only 40 960 lines of 40 steps, so the kernel is
// bound by the latency of a lane's dependent round trips, not by bandwidth.  Tried: U = 1, 2, 4, 8 at 64 lanes per workgroup and 256 lanes per
// workgroup (profiles/scene_scroll.md, section (b)): on the ScanNet-v1 grid the x and y passes gain with every doubling up to 8 (56 VGPRs, still
// 8 waves per SIMD); on the ScanNet-fast grid a call reaches the floor of its two launches at U = 4; the z pass does not care; 256-lane
// workgroups lose on the z pass and gain nothing elsewhere.
#include <algorithm>
#include <vector>

#include "ivx_common.h"

#ifndef IVX_SCROLL_U
#define IVX_SCROLL_U 8
#endif
#ifndef IVX_SCROLL_WG
#define IVX_SCROLL_WG 64
#endif

namespace {

typedef uint32_t word16 __attribute__((ext_vector_type(4)));      // a 16-byte element of the sums: four channels of a voxel, moved as bits
constexpr int SCROLL_MAX_SAMPLES = 32;      // samples per launch: their rows and shifts travel by value in the kernel arguments

struct ScrollArgs {
  void *field[2];                           // blockIdx.z picks the field: the sums alone, or count and (optionally) wsum
  long long row_elems, inner, lines;        // elements per row; elements between two steps of a line; lines per row (outer * inner)
  int32_t L;                                // the length of the axis of this pass
  int32_t row[SCROLL_MAX_SAMPLES];          // blockIdx.y is the sample: its row of the pools ...
  int32_t shift[SCROLL_MAX_SAMPLES];        // ... and its shift along this axis, clamped to [-L, L]
};

// One line p[0], p[st], .. p[(L-1)*st].  UP: s > 0, ascending; else s < 0, descending.  Reads run |s| ahead of writes in walk order (see the top).
// q counts walk steps; at(q) is the q-th position of the walk.  The first n = L - |s| steps copy from |s| steps ahead, the last |s| store zeros.
template <typename T, int U, bool UP>
__device__ __forceinline__ void scroll_line(T *p, const long long st, const int L, const int s) {
  const int ahead = UP ? s : -s, n = L - ahead;                           // (the host clamps |s| to L: n >= 0)
  T *const p0 = UP ? p : p + (long long)(L - 1) * st;                     // the first position of the walk ...
  const long long step = UP ? st : -st;                                   // ... and the way to the next: at(q) = p0[q * step]
  int q = 0;
  for (; q + U <= n; q += U) {                                            // whole blocks: U loads, then U stores
    T v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = p0[(q + u + ahead) * step];
#pragma unroll
    for (int u = 0; u < U; ++u) p0[(q + u) * step] = v[u];
  }
  if (q < n) {                                                            // the last, partial block: the same order, loads before stores
    T v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = q + u < n ? p0[(q + u + ahead) * step] : T{};
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (q + u < n) p0[(q + u) * step] = v[u];
  }
  for (q = n; q < L; ++q) p0[q * step] = T{};                             // the vacated end of the line
}

template <typename T, int U>
__global__ void __launch_bounds__(IVX_SCROLL_WG) volume_scroll_axis_kernel(const ScrollArgs a) {
  const int s = a.shift[blockIdx.y];                                      // uniform per blockIdx.y, like the direction below
  if (s == 0) return;                                                     // nothing moves along this axis: no address is formed
  const long long id = (long long)blockIdx.x * IVX_SCROLL_WG + threadIdx.x;
  if (id >= a.lines) return;                                              // the last, partial workgroup
  const long long o = id / a.inner, i = id - o * a.inner;
  T *p = (T *)a.field[blockIdx.z] + (long long)a.row[blockIdx.y] * a.row_elems + o * a.L * a.inner + i;
  if (s > 0)
    scroll_line<T, U, true>(p, a.inner, a.L, s);
  else
    scroll_line<T, U, false>(p, a.inner, a.L, s);
}

}  // namespace

extern "C" int ivx_volume_scroll_fwd(int32_t B, const int32_t *row, const int32_t *shift, int32_t R, int32_t X, int32_t Y, int32_t Z, int32_t C,
                                     float *volume_sum, int32_t *count, float *wsum, ivx_stream_t stream) {
  const char *what = "ivx_volume_scroll_fwd";
  IVX_REQUIRE(row && shift && volume_sum && count, "%s: null argument (row, shift, volume_sum and count are required; wsum is optional)", what);
  IVX_REQUIRE(B > 0 && R > 0 && X > 0 && Y > 0 && Z > 0 && C > 0, "%s: bad dims (B, R, X, Y, Z and C must be positive)", what);
  IVX_REQUIRE(C % 4 == 0, "%s: C %% 4 must be 0 (the sums move as 16-byte words)", what);
  const long long nvox = (long long)X * Y * Z;
  IVX_REQUIRE(nvox < (1ll << 31), "%s: X*Y*Z must be below 2^31", what);
  IVX_REQUIRE(nvox * (C / 4) / IVX_SCROLL_WG < (1ll << 31) && ((uintptr_t)volume_sum & 15) == 0, "%s: C too large for one grid, or volume_sum not 16-byte aligned", what);
  for (int b = 0; b < B; ++b) IVX_REQUIRE(row[b] >= 0 && row[b] < R, "%s: row[%d] = %d is outside [0, %d)", what, b, row[b], R);
  {
    std::vector<int32_t> sorted(row, row + B);
    std::sort(sorted.begin(), sorted.end());
    const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
    IVX_REQUIRE(dup == sorted.end(), "%s: rows must be distinct (two samples on row %d)", what, dup == sorted.end() ? 0 : *dup);
  }
  const int dims[3] = {X, Y, Z};
  for (int b0 = 0; b0 < B; b0 += SCROLL_MAX_SAMPLES) {
    const int n = std::min(B - b0, SCROLL_MAX_SAMPLES);
    long long outer = 1;
    for (int ax = 0; ax < 3; outer *= dims[ax], ++ax) {                   // x, then y, then z
      ScrollArgs a = {};
      a.L = dims[ax];
      bool any = false;
      for (int b = 0; b < n; ++b) {
        a.row[b] = row[b0 + b];
        a.shift[b] = std::max(-a.L, std::min(a.L, shift[3 * (b0 + b) + ax]));     // |s| >= L zeroes the row whatever its size
        any |= a.shift[b] != 0;
      }
      if (!any) continue;
      const long long after = nvox / (outer * a.L);                       // voxels between two steps along this axis
      for (int words = 0; words < 2; ++words) {                           // the sums as 16-byte elements, then count (and wsum) as 4-byte ones
        const long long e = words ? 1 : C / 4;
        a.row_elems = nvox * e;
        a.inner = after * e;
        a.lines = outer * a.inner;
        a.field[0] = words ? (void *)count : (void *)volume_sum;
        a.field[1] = words ? (void *)wsum : nullptr;
        const dim3 grid((unsigned)((a.lines + IVX_SCROLL_WG - 1) / IVX_SCROLL_WG), (unsigned)n, words && wsum ? 2u : 1u);
        if (words)
          hipLaunchKernelGGL((volume_scroll_axis_kernel<uint32_t, IVX_SCROLL_U>), grid, dim3(IVX_SCROLL_WG), 0, (hipStream_t)stream, a);
        else
          hipLaunchKernelGGL((volume_scroll_axis_kernel<word16, IVX_SCROLL_U>), grid, dim3(IVX_SCROLL_WG), 0, (hipStream_t)stream, a);
        IVX_CHECK_LAUNCH(what);
      }
    }
  }
  return IVX_OK;
}
