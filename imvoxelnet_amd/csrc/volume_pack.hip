// Ordered stream compaction of rows of the scene state pools and its inverse (ivx_volume_pack_fwd / ivx_volume_unpack_fwd, include/imvoxel.h):
// scene snapshots, scene.py.
//
//   kept(n)  <=>  the count word or the wsum word of voxel n is non-zero, compared as raw 32-bit words (-0 and NaN weight sums are kept)
//   pack:    record q of a sample is its q-th kept voxel in ascending flat index: (index, count word, wsum word, payload of C channels)
//   unpack:  every voxel of a named row is written: a listed voxel takes its record, every other becomes unseen (all bits zero)
//
// The F32 payload is the C sums moved as 16-byte words: no float arithmetic touches a value, so every bit pattern survives.  The BF16 payload is
// the mean m = den > 0 ? S / den : +0 (one IEEE division, den the weight sum or (float)count), rounded once to bf16, round to nearest even;
// unpack restores S = float(m) * den, one rounded product.  The file is built with -ffp-contract=off.
//
// Schedule of the pack: three launches per 32 samples, deterministic, no atomics, no spinning, no dependence between workgroups of a launch.
//   1. count   one workgroup of IVX_PACK_WG lanes takes one chunk of IVX_PACK_WG voxels: 8 bytes read per voxel, one __ballot / __popcll per
//              wave, one count per chunk into scratch [B, chunks].
//   2. scan    one workgroup per sample turns its chunk counts into exclusive bases in place (it loops when there are more chunks than lanes)
//              and writes n_out, the true number of kept voxels, whatever cap is.
//   3. write   recomputes the ballots, ranks lane l of a wave by __popcll(m & lanemask(l)) plus the wave and chunk bases, stores index, count
//              and wsum of the records below cap, leaves the chunk's kept voxels in LDS in rank order, and copies the payload with one group of C/4
//              lanes per record: element e of the chunk's payload is record e / (C/4), 16-byte part e % (C/4), so the stores of a workgroup are one
//              contiguous run and the loads are runs of C*4 bytes; IVX_PACK_U elements are in flight per lane.
// The unpack is one launch: a workgroup owns one chunk of voxels, finds the records that fall into it by two binary searches over the
// ascending index list (every probe lies inside [0, n): no address depends on unchecked data), notes them in LDS -- an index outside the chunk
// is skipped, so an index outside the grid is never used -- and writes every voxel of the chunk once, record or zero.
#include <algorithm>
#include <vector>

#include "ivx_common.h"

#ifndef IVX_PACK_WG
#define IVX_PACK_WG 256                      // lanes per workgroup == voxels per chunk
#endif
#ifndef IVX_PACK_U
#define IVX_PACK_U 4                         // 16-byte payload elements in flight per lane
#endif

namespace {

typedef uint32_t word16 __attribute__((ext_vector_type(4)));      // four channels of a voxel, moved as bits
typedef uint16_t half8b __attribute__((ext_vector_type(4)));      // four bf16 means, 8 bytes
constexpr int PACK_MAX_SAMPLES = 32;         // samples per launch: their rows (and record counts) travel by value in the kernel arguments
constexpr int PACK_WAVES = IVX_PACK_WG / 64;
static_assert(IVX_PACK_WG % 64 == 0 && IVX_PACK_WG >= 128, "the unpack's two searches run on lanes 0 and 64");

struct PackArgs {
  const word16 *sum;
  const uint32_t *count, *wsum;              // wsum may be null
  int32_t *scratch, *n_out;                  // [B, chunks] chunk counts, then exclusive bases; [B]
  int32_t *index_out, *count_out;            // [B, cap]
  uint32_t *wsum_out;                        // [B, cap] or null
  void *payload_out;                         // [B, cap, C] fp32 words or bf16
  long long nvox;
  int32_t chunks, C4, cap, b0;               // chunks per row; C / 4; records per sample; the first sample of this launch
  int32_t row[PACK_MAX_SAMPLES];
};

struct UnpackArgs {
  word16 *sum;
  uint32_t *count, *wsum;                    // wsum may be null (then wsum_rec is null too)
  const int32_t *index, *count_rec;          // [B, cap]
  const uint32_t *wsum_rec;
  const void *payload;
  long long nvox;
  int32_t C4, cap, b0;
  int32_t row[PACK_MAX_SAMPLES];
  int32_t n[PACK_MAX_SAMPLES];
};

// The two words that decide whether voxel v of the sample's row is kept; zero beyond the end of the row.
__device__ __forceinline__ bool kept_words(const PackArgs &a, const long long rowoff, const long long v, uint32_t &cw, uint32_t &ww) {
  const bool in = v < a.nvox;
  cw = in ? a.count[rowoff + v] : 0u;
  ww = in && a.wsum ? a.wsum[rowoff + v] : 0u;
  return (cw | ww) != 0u;
}

__global__ void __launch_bounds__(IVX_PACK_WG) volume_pack_count_kernel(const PackArgs a) {
  __shared__ int wave_cnt[PACK_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t cw, ww;
  const bool kept = kept_words(a, (long long)a.row[blockIdx.y] * a.nvox, (long long)blockIdx.x * IVX_PACK_WG + tid, cw, ww);
  const unsigned long long m = __ballot(kept);
  if (lane == 0) wave_cnt[wv] = __popcll(m);
  __syncthreads();
  if (tid == 0) {
    int s = 0;
#pragma unroll
    for (int q = 0; q < PACK_WAVES; ++q) s += wave_cnt[q];
    a.scratch[(long long)(a.b0 + blockIdx.y) * a.chunks + blockIdx.x] = s;
  }
}

// One workgroup per sample: chunk counts -> exclusive bases, in place (a lane reads its element, then writes it); the total goes to n_out.
__global__ void __launch_bounds__(IVX_PACK_WG) volume_pack_scan_kernel(const PackArgs a) {
  __shared__ int wave_tot[PACK_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int32_t *c = a.scratch + (long long)(a.b0 + blockIdx.x) * a.chunks;
  int running = 0;                                                        // (below 2^31: at most X*Y*Z)
  for (int base = 0; base < a.chunks; base += IVX_PACK_WG) {
    const int i = base + tid;
    const int v = i < a.chunks ? c[i] : 0;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < PACK_WAVES; ++q) {
      before += q < wv ? wave_tot[q] : 0;
      tot += wave_tot[q];
    }
    if (i < a.chunks) c[i] = running + before + incl - v;
    running += tot;
    __syncthreads();                                                      // wave_tot is rewritten by the next pass
  }
  if (tid == 0) a.n_out[a.b0 + blockIdx.x] = running;
}

__device__ __forceinline__ uint16_t bf16_rne(const float x) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);      // a NaN stays a NaN
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <bool BF16>
__global__ void __launch_bounds__(IVX_PACK_WG) volume_pack_write_kernel(const PackArgs a) {
  __shared__ int wave_cnt[PACK_WAVES];
  __shared__ int32_t rec_vox[IVX_PACK_WG];                                // the chunk's kept voxels in rank order
  __shared__ float rec_den[IVX_PACK_WG];                                  // BF16: their denominators
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long s = a.b0 + blockIdx.y, rowoff = (long long)a.row[blockIdx.y] * a.nvox;
  const long long v = (long long)blockIdx.x * IVX_PACK_WG + tid;
  uint32_t cw, ww;
  const bool kept = kept_words(a, rowoff, v, cw, ww);
  const unsigned long long m = __ballot(kept);
  if (lane == 0) wave_cnt[wv] = __popcll(m);
  __syncthreads();
  int local = __popcll(m & ((1ULL << lane) - 1ULL)), nk = 0;
#pragma unroll
  for (int q = 0; q < PACK_WAVES; ++q) {
    local += q < wv ? wave_cnt[q] : 0;
    nk += wave_cnt[q];
  }
  const int base = a.scratch[s * a.chunks + blockIdx.x];                  // kept voxels of the sample before this chunk
  const int nw = max(0, min(nk, a.cap - base));                           // records of this chunk below cap: only these are written
  if (kept && local < nw) {
    const long long o = s * a.cap + base + local;
    a.index_out[o] = (int32_t)v;
    a.count_out[o] = (int32_t)cw;
    if (a.wsum_out) a.wsum_out[o] = ww;
    rec_vox[local] = (int32_t)v;
    if (BF16) rec_den[local] = a.wsum ? __uint_as_float(ww) : (float)(int32_t)cw;
  }
  __syncthreads();
  const int total = nw * a.C4;                                            // 16-byte source elements of this chunk's records (<= 256 * C/4)
  const word16 *src = a.sum + rowoff * a.C4;
  const long long dst0 = (s * a.cap + base) * a.C4;
  for (int e0 = tid; e0 < total; e0 += IVX_PACK_WG * IVX_PACK_U) {
    word16 x[IVX_PACK_U];
    float den[IVX_PACK_U];
#pragma unroll
    for (int u = 0; u < IVX_PACK_U; ++u) {
      const int e = e0 + u * IVX_PACK_WG;
      if (e < total) {
        const int r = e / a.C4;
        x[u] = src[(long long)rec_vox[r] * a.C4 + (e - r * a.C4)];
        if (BF16) den[u] = rec_den[r];
      }
    }
#pragma unroll
    for (int u = 0; u < IVX_PACK_U; ++u) {
      const int e = e0 + u * IVX_PACK_WG;
      if (e < total) {
        if (BF16) {
          half8b h;
#pragma unroll
          for (int c = 0; c < 4; ++c) h[c] = bf16_rne(den[u] > 0.f ? __uint_as_float(x[u][c]) / den[u] : 0.f);
          ((half8b *)a.payload_out)[dst0 + e] = h;
        } else {
          ((word16 *)a.payload_out)[dst0 + e] = x[u];
        }
      }
    }
  }
}

// The first position in idx[0, n) whose value is >= v.  Every probe lies inside [0, n), whatever the values are.
__device__ __forceinline__ int lower_bound_idx(const int32_t *idx, const int n, const long long v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((long long)idx[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <bool BF16>
__global__ void __launch_bounds__(IVX_PACK_WG) volume_unpack_kernel(const UnpackArgs a) {
  __shared__ int range[2];
  __shared__ int32_t rec_of[IVX_PACK_WG];                                 // the record of each voxel of the chunk, -1: unseen
  __shared__ float rec_den[IVX_PACK_WG];
  const int tid = threadIdx.x;
  const long long s = a.b0 + blockIdx.y, rowoff = (long long)a.row[blockIdx.y] * a.nvox, rec0 = s * a.cap;
  const long long v0 = (long long)blockIdx.x * IVX_PACK_WG, v1 = min(v0 + IVX_PACK_WG, a.nvox);
  const int n = a.n[blockIdx.y];
  const int32_t *idx = a.index + rec0;                                    // (not dereferenced when n == 0)
  if (tid == 0) range[0] = lower_bound_idx(idx, n, v0);
  if (tid == 64) range[1] = lower_bound_idx(idx, n, v1);
  rec_of[tid] = -1;
  __syncthreads();
  for (int r = range[0] + tid; r < range[1]; r += IVX_PACK_WG) {          // at most 256 records on an ascending list
    const long long i = idx[r];
    if (i >= v0 && i < v1) rec_of[i - v0] = r;                            // anything else is skipped: no address depends on it
  }
  __syncthreads();
  const long long v = v0 + tid;
  if (v < v1) {
    const int r = rec_of[tid];
    const uint32_t cw = r >= 0 ? (uint32_t)a.count_rec[rec0 + r] : 0u;
    const uint32_t ww = r >= 0 && a.wsum_rec ? a.wsum_rec[rec0 + r] : 0u;
    a.count[rowoff + v] = cw;
    if (a.wsum) a.wsum[rowoff + v] = ww;
    if (BF16) rec_den[tid] = a.wsum_rec ? __uint_as_float(ww) : (float)(int32_t)cw;
  }
  if (BF16) __syncthreads();
  const int total = (int)(v1 - v0) * a.C4;
  word16 *dst = a.sum + (rowoff + v0) * a.C4;
  for (int e0 = tid; e0 < total; e0 += IVX_PACK_WG * IVX_PACK_U) {
    word16 x[IVX_PACK_U];
#pragma unroll
    for (int u = 0; u < IVX_PACK_U; ++u) {
      const int e = e0 + u * IVX_PACK_WG;
      x[u] = word16{0u, 0u, 0u, 0u};
      if (e < total) {
        const int l = e / a.C4, part = e - l * a.C4, r = rec_of[l];
        if (r >= 0) {
          if (BF16) {
            const half8b h = ((const half8b *)a.payload)[(rec0 + r) * a.C4 + part];
            const float den = rec_den[l];
#pragma unroll
            for (int c = 0; c < 4; ++c) x[u][c] = __float_as_uint(__uint_as_float((uint32_t)h[c] << 16) * den);
          } else {
            x[u] = ((const word16 *)a.payload)[(rec0 + r) * a.C4 + part];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < IVX_PACK_U; ++u) {
      const int e = e0 + u * IVX_PACK_WG;
      if (e < total) dst[e] = x[u];
    }
  }
}

// The checks the two entries share.  Returns IVX_OK or sets the message and returns IVX_ERR_INVALID_ARG.
int check_rows(const char *what, int32_t B, const int32_t *row, int32_t R, int32_t X, int32_t Y, int32_t Z, int32_t C, const void *volume_sum,
               int32_t payload_dtype, const void *payload, int32_t cap) {
  IVX_REQUIRE(B > 0 && R > 0 && X > 0 && Y > 0 && Z > 0 && C > 0, "%s: bad dims (B, R, X, Y, Z and C must be positive)", what);
  IVX_REQUIRE(C % 4 == 0, "%s: C %% 4 must be 0 (the sums move as 16-byte words)", what);
  IVX_REQUIRE((long long)X * Y * Z < (1ll << 31), "%s: X*Y*Z must be below 2^31", what);
  IVX_REQUIRE(payload_dtype == IVX_F32 || payload_dtype == IVX_BF16, "%s: unknown payload_dtype %d (IVX_F32 or IVX_BF16)", what, payload_dtype);
  IVX_REQUIRE(cap >= 0, "%s: cap must not be negative, got %d", what, cap);
  IVX_REQUIRE(((uintptr_t)volume_sum & 15) == 0, "%s: volume_sum must be 16-byte aligned", what);
  IVX_REQUIRE(((uintptr_t)payload & (payload_dtype == IVX_BF16 ? 7 : 15)) == 0, "%s: the payload must be 16-byte aligned (8-byte aligned for bf16)", what);
  for (int b = 0; b < B; ++b) IVX_REQUIRE(row[b] >= 0 && row[b] < R, "%s: row[%d] = %d is outside [0, %d)", what, b, row[b], R);
  std::vector<int32_t> sorted(row, row + B);
  std::sort(sorted.begin(), sorted.end());
  const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
  IVX_REQUIRE(dup == sorted.end(), "%s: rows must be distinct (two samples on row %d)", what, dup == sorted.end() ? 0 : *dup);
  return IVX_OK;
}

long long pack_chunks(long long nvox) { return (nvox + IVX_PACK_WG - 1) / IVX_PACK_WG; }

}  // namespace

extern "C" int64_t ivx_volume_pack_scratch_bytes(int32_t B, int32_t X, int32_t Y, int32_t Z) {
  if (B <= 0 || X <= 0 || Y <= 0 || Z <= 0 || (long long)X * Y * Z >= (1ll << 31)) return IVX_ERR_INVALID_ARG;
  return ivx_align_up((int64_t)B * pack_chunks((long long)X * Y * Z) * (int64_t)sizeof(int32_t), 256);
}

extern "C" int ivx_volume_pack_fwd(int32_t B, const int32_t *row, int32_t R, int32_t X, int32_t Y, int32_t Z, int32_t C, const float *volume_sum,
                                   const int32_t *count, const float *wsum, int32_t payload_dtype, int32_t cap, int32_t *index_out, void *payload_out,
                                   float *wsum_out, int32_t *count_out, int32_t *n_out, void *scratch, ivx_stream_t stream) {
  const char *what = "ivx_volume_pack_fwd";
  IVX_REQUIRE(row && volume_sum && count && n_out, "%s: null argument (row, volume_sum, count and n_out are required; wsum is optional)", what);
  IVX_REQUIRE(scratch, "%s: null scratch (ivx_volume_pack_scratch_bytes tells its size)", what);
  if (const int rc = check_rows(what, B, row, R, X, Y, Z, C, volume_sum, payload_dtype, payload_out, cap)) return rc;
  IVX_REQUIRE(cap == 0 || (index_out && payload_out && count_out), "%s: cap > 0 with a null output (index_out, payload_out and count_out are required)", what);
  IVX_REQUIRE(cap == 0 || (wsum != nullptr) == (wsum_out != nullptr), "%s: wsum and wsum_out must both be given or both be NULL", what);
  const long long nvox = (long long)X * Y * Z;
  for (int b0 = 0; b0 < B; b0 += PACK_MAX_SAMPLES) {
    const int nb = std::min(B - b0, PACK_MAX_SAMPLES);
    PackArgs a = {};
    a.sum = (const word16 *)volume_sum;
    a.count = (const uint32_t *)count;
    a.wsum = (const uint32_t *)wsum;
    a.scratch = (int32_t *)scratch;
    a.n_out = n_out;
    a.index_out = index_out;
    a.count_out = count_out;
    a.wsum_out = (uint32_t *)wsum_out;
    a.payload_out = payload_out;
    a.nvox = nvox;
    a.chunks = (int32_t)pack_chunks(nvox);
    a.C4 = C / 4;
    a.cap = cap;
    a.b0 = b0;
    for (int b = 0; b < nb; ++b) a.row[b] = row[b0 + b];
    const dim3 grid((unsigned)a.chunks, (unsigned)nb), wg(IVX_PACK_WG);
    hipLaunchKernelGGL(volume_pack_count_kernel, grid, wg, 0, (hipStream_t)stream, a);
    IVX_CHECK_LAUNCH(what);
    hipLaunchKernelGGL(volume_pack_scan_kernel, dim3((unsigned)nb), wg, 0, (hipStream_t)stream, a);
    IVX_CHECK_LAUNCH(what);
    if (cap == 0) continue;                                               // the count-only form
    if (payload_dtype == IVX_BF16)
      hipLaunchKernelGGL(volume_pack_write_kernel<true>, grid, wg, 0, (hipStream_t)stream, a);
    else
      hipLaunchKernelGGL(volume_pack_write_kernel<false>, grid, wg, 0, (hipStream_t)stream, a);
    IVX_CHECK_LAUNCH(what);
  }
  return IVX_OK;
}

extern "C" int ivx_volume_unpack_fwd(int32_t B, const int32_t *row, const int32_t *n, int32_t cap, const int32_t *index, const void *payload,
                                     const float *wsum_rec, const int32_t *count_rec, int32_t payload_dtype, int32_t R, int32_t X, int32_t Y, int32_t Z,
                                     int32_t C, float *volume_sum, int32_t *count, float *wsum, ivx_stream_t stream) {
  const char *what = "ivx_volume_unpack_fwd";
  IVX_REQUIRE(row && n && volume_sum && count, "%s: null argument (row, n, volume_sum and count are required; wsum is optional)", what);
  if (const int rc = check_rows(what, B, row, R, X, Y, Z, C, volume_sum, payload_dtype, payload, cap)) return rc;
  IVX_REQUIRE(cap == 0 || (index && payload && count_rec), "%s: cap > 0 with a null record list (index, payload and count_rec are required)", what);
  IVX_REQUIRE(cap == 0 ? !wsum_rec || wsum : (wsum != nullptr) == (wsum_rec != nullptr), "%s: wsum and wsum_rec must both be given or both be NULL", what);
  for (int b = 0; b < B; ++b) IVX_REQUIRE(n[b] >= 0 && n[b] <= cap, "%s: n[%d] = %d is outside [0, cap = %d]", what, b, n[b], cap);
  const long long nvox = (long long)X * Y * Z;
  for (int b0 = 0; b0 < B; b0 += PACK_MAX_SAMPLES) {
    const int nb = std::min(B - b0, PACK_MAX_SAMPLES);
    UnpackArgs a = {};
    a.sum = (word16 *)volume_sum;
    a.count = (uint32_t *)count;
    a.wsum = (uint32_t *)wsum;
    a.index = index;
    a.count_rec = count_rec;
    a.wsum_rec = (const uint32_t *)wsum_rec;
    a.payload = payload;
    a.nvox = nvox;
    a.C4 = C / 4;
    a.cap = cap;
    a.b0 = b0;
    for (int b = 0; b < nb; ++b) {
      a.row[b] = row[b0 + b];
      a.n[b] = n[b0 + b];
    }
    const dim3 grid((unsigned)pack_chunks(nvox), (unsigned)nb), wg(IVX_PACK_WG);
    if (payload_dtype == IVX_BF16)
      hipLaunchKernelGGL(volume_unpack_kernel<true>, grid, wg, 0, (hipStream_t)stream, a);
    else
      hipLaunchKernelGGL(volume_unpack_kernel<false>, grid, wg, 0, (hipStream_t)stream, a);
    IVX_CHECK_LAUNCH(what);
  }
  return IVX_OK;
}
